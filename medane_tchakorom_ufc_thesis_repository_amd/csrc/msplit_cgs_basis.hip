// msplit_cgs_basis.hip -- the classical Gram-Schmidt (CGS) kernels of GMRES over a Krylov basis that is not the plain
// f64 one of msplit_k_dot*.hip / msplit_k_maxpy.hip, for gfx950: the basis stored as float (MSP_BASIS_F32), as 16-bit
// integers with one exponent per chunk (MSP_BASIS_B16), and the f64 basis under a left Jacobi preconditioner
// (MSP_PC_JACOBI).  Each kernel is written once, over two compile-time policies:
//   the basis format F (F32, B16, F64): how a stored element becomes (value * sc[j]) and how a vector is rounded
//                                       and stored;
//   the W loader (WPlain, WDinv):       W as it is, or W .* dinv formed as it is loaded.
// Instantiated are the combinations the solver has: {F32, B16} x WPlain (store, mdot, maxpy_norm, accum) and
// F64 x WDinv (store, mdot, maxpy_norm); a compressed basis under Jacobi is refused in ksp_gmres.c.
//
// What every instantiation shares -- the bitwise contract: only storage differs, every value is a double once it is
// loaded and all arithmetic is the f64 path's, statement for statement (-ffp-contract=off, the DBR reduction order of
// msplit_kdev.hpp, PETSc's VecMAXPY grouping, (value * sc[j]) as its own multiply).  A vector is rounded once, when
// it is stored, and its norm is taken of the values read back -- what is in memory is the vector.
//
// Lane map (the DBR map): workgroup c owns elements [4096c, 4096c + 4096), lane t owns base + j*512 + 2t, +1 for
// j = 0..7; sums are per-lane sequential, then the wave64 butterfly, then (w0 + w1) + (w2 + w3) into
// partial[v * nchunks + c].  Stage 2 is msk_dot_stage2 / mspi_gm_norm_update, unchanged.  A partial last chunk (and
// odd n) takes the guarded element-wise path; nothing is read or written at or beyond n.  Basis loads are
// non-temporal in a full chunk (the basis streams through once per kernel and is far larger than the MALL) and plain
// in the guarded path.
//
// F32: one float2 per slice (the basis stride is a multiple of 1024 floats, so every float2 is aligned).
//   rnd(v) = (double)(float)v -- round to nearest even, gradual underflow, overflow to +-inf (v_cvt_f32_f64 under the
//   kernel's default mode: f32 denormals are kept on gfx950 code objects).  A vector is stored twice: as f32 to vout
//   (non-temporal) and as f64 to cur, the next MatMult's input (plain).
//
// B16: per chunk c of a vector (elements [4096c, min(4096(c+1), n))), exponents eb[v * nchunks + c], int32:
//   any element NaN or +-inf   every element reads back NaN; the stored exponent is kNonFinite
//   M = max |v_i| == 0         every element reads back +0.0
//   otherwise                  M = m 2^E, 0.5 <= m < 1 (frexp; subnormal M included, E >= -1073),
//                              q_i = clamp(rint(ldexp(v_i, 15 - E)), -32767, 32767)   (rint: ties to even),
//                              s_i = ldexp(q_i, E - 15)                               (IEEE ldexp, v_ldexp_f64)
//   The workgroup that stores a vector holds the whole chunk in registers, so M costs one more workgroup reduction
//   (one barrier, executed by every lane) and no pass.  M and the non-finite test are one reduction: the maximum of
//   the |v_i| bit patterns as unsigned integers orders finite doubles as fmax does and puts inf and every NaN above
//   them (fmax would drop NaN).  Stored twice, as F32: int16 to vout / eout, f64 to cur.
//   Layout inside a full chunk: two lane-contiguous halves -- the element at (lane t, slice j, half k) is int16
//   4096c + 2048 (j / 4) + 8t + 2 (j % 4) + k, so a lane fetches its 16 values with two 16-byte non-temporal loads,
//   each of them fully coalesced (a wave covers 1 KiB contiguous per load, the workgroup 4 KiB).  Keeping a lane's
//   32 bytes contiguous instead (16t + 2j + k: every load touches half of each 128-byte line) measured 4.85 against
//   5.95 TB/s in the MAXPY, 256^3.  A partial last chunk is stored in natural order, element e at int16 e -- the
//   permutation of a full chunk would scatter it beyond n -- so the pad [n, stride) stays untouched with a stride of
//   n rounded up to 2048 int16 (4 KiB).  The layout is private to this file: nothing else reads a block16 basis.
//
// F64 with WDinv: PETSc's PCJACOBI (-pc_jacobi_type diagonal) on the left with the preconditioned residual norm:
//   PCSetUp   dinv_i = 1 / a_ii (one f64 division); 1.0 where row i stores no diagonal entry or a_ii == +-0.0
//   PCApply   z_i = r_i * dinv_i (VecPointwiseMult: one f64 multiply, never a division, never contracted)
//   The MatMult stores the raw W = A (sc[it] VV(it)) and both CGS kernels form w = W .* dinv in registers as they
//   load W (one multiply per element, before any product), so the raw W is never rewritten and the preconditioner
//   costs one more 8-byte read per row in each kernel.  One double2 per slice, nothing is rounded, and there is no
//   second copy: the MAXPY stores VV(it+1) non-temporally, apply_norm stores z with a plain store.
//
// Aliasing: vout / eout are another vector of the basis vb / another row of eb, and in round_store / apply_norm r
// may be the vector that is written (each lane reads its own elements before it writes them) -- none of those is
// restrict.  The kernels at the end of the file are thin: they carry the argument lists and __restrict__ (which
// kernel arguments passed as structs would lose -- the MDot tails then wait for all their loads at once).
#include <type_traits>

#include "msplit_kdev.hpp"

namespace {

using namespace msk;  // kT, kIters, kChunk, stopped, wave_butterfly, dx2, ix4

static_assert(MSK_CB_MAX_GROUP <= kT, "one lane per vector writes the chunk's partials");

// (w0 + w1) + (w2 + w3) of one value per lane into out[0] (lane 0 of the workgroup)
__device__ __forceinline__ void block_fold(double v, double* red, double* out) {
  const int t = threadIdx.x;
  v = wave_butterfly(v);
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  if (t == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------ W loaders
// at: element e as the kernels see it; at2: the aligned pair at e
struct WPlain {
  const double* w;
  __device__ __forceinline__ double at(int64_t e) const { return w[e]; }
  __device__ __forceinline__ double2 at2(int64_t e) const { return *reinterpret_cast<const double2*>(w + e); }
};
struct WDinv {  // PCApply as the vector is loaded
  const double* w;
  const double* dinv;
  __device__ __forceinline__ double at(int64_t e) const { return w[e] * dinv[e]; }
  __device__ __forceinline__ double2 at2(int64_t e) const {
    const double2 q = *reinterpret_cast<const double2*>(w + e), d = *reinterpret_cast<const double2*>(dinv + e);
    return make_double2(q.x * d.x, q.y * d.y);
  }
};

// the lane's 16 values of W (WDinv: of W .* dinv) at its DBR positions (0 at and beyond n)
template <class W>
__device__ __forceinline__ void load_w(const W& a, int64_t base, int64_t n, bool full, double (&wr)[2 * kIters]) {
  if (full) {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const double2 q = a.at2(base + j * (2 * kT));
      wr[2 * j] = q.x;
      wr[2 * j + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      wr[2 * j] = e < n ? a.at(e) : 0.0;
      wr[2 * j + 1] = e + 1 < n ? a.at(e + 1) : 0.0;
    }
  }
}

// -------------------------------------------------------------- basis formats
// A format supplies:
//   Basis, Out   the kernels' arguments: the stored basis, and where a new vector goes
//   Vec          one vector's wave-uniform state in chunk c (vec builds it)
//   Chunk        a lane's 16 raw values of a full chunk (fetch: non-temporal loads)
//   val          a stored element as its scaled double, value * sc[j]
//   half         the same of half k of slice j of a Chunk
//   open         the MDot's per-vector prologue: Vec and Chunk, in the format's own order
//   kDotGroup    the MDot's largest group
//   kPrefetch    whether the MAXPY fetches a group's Chunks before the first product or loads slice by slice (ld).
//                The compiler follows the source here: F32's MAXPY + norm takes 174 VGPRs written the first way
//                and 198 the second, which is the measured one
//   write        rounds and stores the lane's 16 values; returns its part of the sum of squares of what it stored,
//                in dot_chunk's SELF order
template <class T>
struct PlainOut;
template <>
struct PlainOut<float> {
  double* cur;
  float* vout;
};
template <>
struct PlainOut<double> {
  double* vout;
};

template <class T>
struct Plain {
  typedef T T2 __attribute__((ext_vector_type(2)));
  static constexpr int kDotGroup = 4;
  static constexpr bool kPrefetch = false;
  static constexpr bool kCur = std::is_same_v<T, float>;  // a rounded format keeps the f64 copy for the MatMult
  struct Basis {
    const T* vb;
    int64_t stride;
  };
  typedef PlainOut<T> Out;
  struct Vec {
    const T* y;
    double sv;
  };
  struct Chunk {
    T2 q[kIters];
  };

  static __device__ __forceinline__ Vec vec(const Basis& B, const double* __restrict__ scale, int v, int64_t) {
    return {B.vb + (int64_t)v * B.stride, scale[v]};
  }
  static __device__ __forceinline__ T2 ld(const T* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const T2*>(p));
  }
  static __device__ __forceinline__ Chunk fetch(const T* y, int64_t, int64_t base) {
    Chunk q;
#pragma unroll
    for (int j = 0; j < kIters; ++j) q.q[j] = ld(y + base + j * (2 * kT));
    return q;
  }
  // the MDot's per-vector prologue: the state first, then the loads
  static __device__ __forceinline__ void open(const Basis& B, const double* __restrict__ scale, int v, int64_t c,
                                              int64_t base, Vec& y, Chunk& q) {
    y = vec(B, scale, v, c);
    q = fetch(y.y, c, base);
  }
  static __device__ __forceinline__ double val(T x, const Vec& y) { return (double)x * y.sv; }
  static __device__ __forceinline__ double half(const Chunk& q, const Vec& y, int j, int k) {
    return val(k ? q.q[j].y : q.q[j].x, y);
  }

  // NT: F64 only (see the header) -- F32's vout is always non-temporal, its cur always plain
  template <bool NT>
  static __device__ __forceinline__ double write(const double (&u)[2 * kIters], const Out& o, int64_t c, int64_t base,
                                                 int64_t n, bool full) {
    double acc = 0.0;
    if (full) {
#pragma unroll
      for (int j = 0; j < kIters; ++j) {
        const int64_t e = base + j * (2 * kT);
        T2 f;
        f.x = (T)u[2 * j];
        f.y = (T)u[2 * j + 1];
        const double d0 = (double)f.x, d1 = (double)f.y;
        if constexpr (NT || kCur) __builtin_nontemporal_store(f, reinterpret_cast<T2*>(o.vout + e));
        else *reinterpret_cast<T2*>(o.vout + e) = f;
        if constexpr (kCur) *reinterpret_cast<double2*>(o.cur + e) = make_double2(d0, d1);
        acc = acc + d0 * d0;
        acc = acc + d1 * d1;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 2 * kIters; ++j) {
        const int64_t e = base + (j >> 1) * (2 * kT) + (j & 1);
        if (e < n) {
          const T f = (T)u[j];
          const double d = (double)f;
          o.vout[e] = f;
          if constexpr (kCur) o.cur[e] = d;
          acc = acc + d * d;
        }
      }
    }
    return acc;
  }
};
typedef Plain<float> F32;
typedef Plain<double> F64;

constexpr int32_t kNonFinite = INT32_MIN;  // the exponent of a chunk that held a NaN or an inf
constexpr unsigned long long kAbsMask = 0x7fffffffffffffffull, kInfBits = 0x7ff0000000000000ull;

// The chunk's exponent from the 16 values of every lane (0 at and beyond n): E of M = m 2^E, 0 for a zero chunk,
// kNonFinite if any value is NaN or inf.  The maximum is order-free, so the butterfly and the four values through
// LDS are exact.  One barrier, which every lane of the workgroup must reach; the result is workgroup-uniform.
__device__ __forceinline__ int32_t chunk_exponent(const double (&u)[2 * kIters]) {
  __shared__ unsigned long long mred[4];
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

struct B16 {
  static constexpr int kDotGroup = 8;  // then one group of four: 2G 16-byte loads in flight per lane
  static constexpr bool kPrefetch = true;
  struct Basis {
    const int16_t* vb;
    int64_t stride;
    const int32_t* eb;
    int64_t nchunks;
  };
  struct Out {
    double* cur;
    int16_t* vout;
    int32_t* eout;
  };
  struct Vec {  // value = ldexp(q, k) * sv, sv = NaN for a non-finite chunk
    const int16_t* y;
    int k;
    double sv;
  };
  // dword j holds (slice j, half 0) in its low and (slice j, half 1) in its high 16 bits; a = slices 0..3 (the
  // chunk's first 4 KiB), b = slices 4..7 (its second)
  struct Chunk {
    ix4 a, b;
  };

  static __device__ __forceinline__ Vec vec(const Basis& B, const double* __restrict__ scale, int v, int64_t c) {
    const int32_t e = B.eb[(int64_t)v * B.nchunks + c];
    const double s = scale[v];
    return {B.vb + (int64_t)v * B.stride, e == kNonFinite ? 0 : e - 15, e == kNonFinite ? __builtin_nan("") : s};
  }
  static __device__ __forceinline__ Chunk fetch(const int16_t* y, int64_t c, int64_t) {
    const int16_t* p = y + c * kChunk + 8 * (int)threadIdx.x;
    Chunk q;
    q.a = __builtin_nontemporal_load(reinterpret_cast<const ix4*>(p));
    q.b = __builtin_nontemporal_load(reinterpret_cast<const ix4*>(p + kChunk / 2));
    return q;
  }
  // the MDot's per-vector prologue: the two loads first, then the exponent and the scale -- written the other way
  // round the compiler keeps 114 VGPRs for 132 and the kernel measured 3 to 4 % slower, 256^3
  static __device__ __forceinline__ void open(const Basis& B, const double* __restrict__ scale, int v, int64_t c,
                                              int64_t base, Vec& y, Chunk& q) {
    q = fetch(B.vb + (int64_t)v * B.stride, c, base);
    y = vec(B, scale, v, c);
  }
  static __device__ __forceinline__ double val(int q, const Vec& y) { return ldexp((double)q, y.k) * y.sv; }
  static __device__ __forceinline__ double half(const Chunk& q, const Vec& y, int j, int k) {
    const int d = j < 4 ? q.a[j & 3] : q.b[j & 3];
    return val(k ? d >> 16 : (int)(int16_t)(d & 0xffff), y);
  }

  template <bool>
  static __device__ __forceinline__ double write(const double (&u)[2 * kIters], const Out& o, int64_t c, int64_t base,
                                                 int64_t n, bool full) {
    const int t = threadIdx.x;
    const int32_t E = chunk_exponent(u);
    if (t == 0) o.eout[c] = E;
    double acc = 0.0;
    if (full) {
      int dw[kIters];
#pragma unroll
      for (int j = 0; j < kIters; ++j) {
        const int64_t e = base + j * (2 * kT);
        double d0, d1;
        const int q0 = quantise(u[2 * j], E, &d0), q1 = quantise(u[2 * j + 1], E, &d1);
        dw[j] = (q0 & 0xffff) | (int)((unsigned)q1 << 16);
        *reinterpret_cast<double2*>(o.cur + e) = make_double2(d0, d1);
        acc = acc + d0 * d0;
        acc = acc + d1 * d1;
      }
      ix4 a, b;
      a.x = dw[0], a.y = dw[1], a.z = dw[2], a.w = dw[3];
      b.x = dw[4], b.y = dw[5], b.z = dw[6], b.w = dw[7];
      __builtin_nontemporal_store(a, reinterpret_cast<ix4*>(o.vout + c * kChunk + 8 * t));
      __builtin_nontemporal_store(b, reinterpret_cast<ix4*>(o.vout + c * kChunk + kChunk / 2 + 8 * t));
    } else {
#pragma unroll
      for (int j = 0; j < 2 * kIters; ++j) {
        const int64_t e = base + (j >> 1) * (2 * kT) + (j & 1);
        if (e < n) {
          double d;
          o.vout[e] = (int16_t)quantise(u[j], E, &d);
          o.cur[e] = d;
          acc = acc + d * d;
        }
      }
    }
    return acc;
  }
};

// ------------------------------------------------------------ round and store
// F32 / B16 round_store: cur = rnd(r) as f64, vout (/ eout) = the same values in the format; F64 apply_norm:
// z = r .* dinv.  partial[c] = this chunk's DBR partial of the sum of squares of what was stored.
template <class F, class W>
__device__ __forceinline__ void cgs_store(const W& r, const typename F::Out& o, int64_t n, double* partial,
                                           const int* stop) {
  if (stopped(stop)) return;
  __shared__ double red[4];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double u[2 * kIters];
  load_w(r, base, n, full, u);
  block_fold(F::template write<false>(u, o, c, base, n, full), red, partial + c);
}

// ----------------------------------------------------------------------- MDot
// G vectors of a full chunk at once: all their loads are issued before the first product (dot_group_full's shape),
// then G independent accumulations in dot_chunk's order, acc += w * (v * sc).
template <class F, int G>
__device__ __forceinline__ void dot_group(const double (&wr)[2 * kIters], const typename F::Basis& B,
                                          const double* __restrict__ scale, int g, int64_t c, int64_t base,
                                          double (*red)[4]) {
  const int t = threadIdx.x;
  typename F::Vec y[G];
  typename F::Chunk q[G];
#pragma unroll
  for (int u = 0; u < G; ++u) F::open(B, scale, g + u, c, base, y[u], q[u]);
  double acc[G];
#pragma unroll
  for (int u = 0; u < G; ++u) {
    acc[u] = 0.0;
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      acc[u] = acc[u] + wr[2 * j] * F::half(q[u], y[u], j, 0);
      acc[u] = acc[u] + wr[2 * j + 1] * F::half(q[u], y[u], j, 1);
    }
  }
#pragma unroll
  for (int u = 0; u < G; ++u) {
    acc[u] = wave_butterfly(acc[u]);
    if ((t & 63) == 0) red[g + u][t >> 6] = acc[u];
  }
}

// partial[v * nchunks + c] = chunk c of w . (sc[v] VV(v)), v < nv <= MSK_CB_MAX_GROUP; w stays in registers while
// the nv vectors stream past in groups of F::kDotGroup (8: then one group of four), then the 3/2/1 tail.
// #pragma unroll 1 on the group loop holds the register budget.
template <class F, class W>
__device__ __forceinline__ void cgs_mdot(const W& w, const typename F::Basis& B, const double* scale, int nv,
                                          int64_t n, double* partial, int64_t nchunks, const int* stop) {
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
    for (; g + F::kDotGroup <= nv; g += F::kDotGroup) dot_group<F, F::kDotGroup>(wr, B, scale, g, c, base, red);
    if constexpr (F::kDotGroup == 8) {
      if (g + 4 <= nv) {
        dot_group<F, 4>(wr, B, scale, g, c, base, red);
        g += 4;
      }
    }
    const int rem = nv - g;  // uniform
    if (rem == 3) dot_group<F, 3>(wr, B, scale, g, c, base, red);
    else if (rem == 2) dot_group<F, 2>(wr, B, scale, g, c, base, red);
    else if (rem == 1) dot_group<F, 1>(wr, B, scale, g, c, base, red);
  } else {
#pragma unroll 1
    for (int v = 0; v < nv; ++v) {
      const typename F::Vec y = F::vec(B, scale, v, c);
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < kIters; ++j) {
        const int64_t e = base + j * (2 * kT);
        if (e < n) acc = acc + wr[2 * j] * F::val(y.y[e], y);
        if (e + 1 < n) acc = acc + wr[2 * j + 1] * F::val(y.y[e + 1], y);
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
// The coefficients are adev's, negated with NEG.
template <class F, int G, bool FULL, bool NEG>
__device__ __forceinline__ void axpy_group(double (&u)[2 * kIters], const typename F::Basis& B,
                                           const double* __restrict__ scale, const double* __restrict__ adev, int g,
                                           int64_t c, int64_t base, int64_t n) {
  double a[G];
  typename F::Vec y[G];
  typename F::Chunk qv[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {  // wave-uniform but for the loads
    const double aq = adev[g + q];
    a[q] = NEG ? -aq : aq;
    y[q] = F::vec(B, scale, g + q, c);
    if constexpr (FULL && F::kPrefetch) qv[q] = F::fetch(y[q].y, c, base);
  }
#pragma unroll
  for (int j = 0; j < kIters; ++j) {
    const int64_t e = base + j * (2 * kT);
    double p0[G], p1[G];
#pragma unroll
    for (int q = 0; q < G; ++q) {
      if constexpr (FULL && F::kPrefetch) {
        p0[q] = F::half(qv[q], y[q], j, 0);
        p1[q] = F::half(qv[q], y[q], j, 1);
      } else if constexpr (FULL) {
        const auto v = F::ld(y[q].y + e);
        p0[q] = F::val(v.x, y[q]);
        p1[q] = F::val(v.y, y[q]);
      } else {
        p0[q] = e < n ? F::val(y[q].y[e], y[q]) : 0.0;
        p1[q] = e + 1 < n ? F::val(y[q].y[e + 1], y[q]) : 0.0;
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
template <class F, bool FULL, bool NEG>
__device__ __forceinline__ void maxpy_body(double (&u)[2 * kIters], const typename F::Basis& B,
                                             const double* __restrict__ scale, const double* __restrict__ adev,
                                             int nv, int64_t c, int64_t base, int64_t n) {
  const int jrem = nv & 3;
  if (jrem == 3) axpy_group<F, 3, FULL, NEG>(u, B, scale, adev, 0, c, base, n);
  else if (jrem == 2) axpy_group<F, 2, FULL, NEG>(u, B, scale, adev, 0, c, base, n);
  else if (jrem == 1) axpy_group<F, 1, FULL, NEG>(u, B, scale, adev, 0, c, base, n);
  // one group of four per iteration: F32 has 32 float2 loads in flight per lane at 198 VGPRs (two workgroups per
  // CU); two groups per iteration take 298 VGPRs, one workgroup per CU
#pragma unroll 1
  for (int g = jrem; g < nv; g += 4) axpy_group<F, 4, FULL, NEG>(u, B, scale, adev, g, c, base, n);
}

// w' = w - sum_j h_j (sc[j] VV(j)) (coefficients adev, negated), rounded and stored as the new basis vector (and to
// cur where the format has one); partial[c] = the chunk's DBR partial of the sum of squares of what was stored.
// win stays as the MatMult wrote it.
template <class F, class W>
__device__ __forceinline__ void cgs_maxpy_norm(const W& win, const typename F::Out& o, const typename F::Basis& B,
                                                const double* scale, const double* adev, int nv, int64_t n,
                                                double* partial, const int* stop) {
  if (stopped(stop)) return;
  __shared__ double red[4];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double u[2 * kIters];
  load_w(win, base, n, full, u);
  if (full) maxpy_body<F, true, true>(u, B, scale, adev, nv, c, base, n);
  else maxpy_body<F, false, true>(u, B, scale, adev, nv, c, base, n);
  block_fold(F::template write<true>(u, o, c, base, n, full), red, partial + c);
}

// BuildSoln: x = x + (0 + sum_j nrs_j (sc[j] VV(j))), the vector count read from the device (*nvdev; 0: nothing)
template <class F>
__device__ __forceinline__ void cgs_accum(double* x, const int* nvdev, const typename F::Basis& B,
                                           const double* scale, const double* coef, int64_t n, const int* stop) {
  if (stopped(stop)) return;
  const int nv = *nvdev;
  if (nv <= 0) return;
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  double u[2 * kIters];
#pragma unroll
  for (int j = 0; j < 2 * kIters; ++j) u[j] = 0.0;
  if ((c + 1) * kChunk <= n) {
    maxpy_body<F, true, false>(u, B, scale, coef, nv, c, base, n);
#pragma unroll
    for (int j = 0; j < kIters; ++j) {  // VecAXPY(x, 1.0, T): x + T
      const int64_t e = base + j * (2 * kT);
      const double2 q = *reinterpret_cast<const double2*>(x + e);
      *reinterpret_cast<double2*>(x + e) = make_double2(q.x + u[2 * j], q.y + u[2 * j + 1]);
    }
  } else {
    maxpy_body<F, false, false>(u, B, scale, coef, nv, c, base, n);
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      if (e < n) x[e] = x[e] + u[2 * j];
      if (e + 1 < n) x[e + 1] = x[e + 1] + u[2 * j + 1];
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

// -------------------------------------------------------------------- kernels
// The instantiations, one line of body each.  The argument lists are the launchers'; __restrict__ is on every pointer
// but those named under Aliasing in the header.
#define KERNEL __global__ __launch_bounds__(kT) void
#define R __restrict__

KERNEL k_cb_round_store(const double* r, double* cur, float* R v0, int64_t n, double* R partial, const int* R stop) {
  cgs_store<F32>(WPlain{r}, F32::Out{cur, v0}, n, partial, stop);
}
KERNEL k_cb_mdot(const double* R w, const float* R vb, int64_t stride, const double* R scale, int nv, int64_t n,
                 double* R partial, int64_t nchunks, const int* R stop) {
  cgs_mdot<F32>(WPlain{w}, F32::Basis{vb, stride}, scale, nv, n, partial, nchunks, stop);
}
KERNEL k_cb_maxpy_norm(const double* R win, double* R cur, float* vout, const float* vb, int64_t stride,
                       const double* R scale, const double* R adev, int nv, int64_t n, double* R partial,
                       const int* R stop) {
  cgs_maxpy_norm<F32>(WPlain{win}, F32::Out{cur, vout}, F32::Basis{vb, stride}, scale, adev, nv, n, partial, stop);
}
KERNEL k_cb_accum(double* R x, const int* R nvdev, const float* R vb, int64_t stride, const double* R scale,
                  const double* R coef, int64_t n, const int* R stop) {
  cgs_accum<F32>(x, nvdev, F32::Basis{vb, stride}, scale, coef, n, stop);
}

KERNEL k_cb16_round_store(const double* r, double* cur, int16_t* R v0, int32_t* R e0, int64_t n, double* R partial,
                          const int* R stop) {
  cgs_store<B16>(WPlain{r}, B16::Out{cur, v0, e0}, n, partial, stop);
}
KERNEL k_cb16_mdot(const double* R w, const int16_t* R vb, int64_t stride, const int32_t* R eb, const double* R scale,
                   int nv, int64_t n, double* R partial, int64_t nchunks, const int* R stop) {
  cgs_mdot<B16>(WPlain{w}, B16::Basis{vb, stride, eb, nchunks}, scale, nv, n, partial, nchunks, stop);
}
KERNEL k_cb16_maxpy_norm(const double* R win, double* R cur, int16_t* vout, int32_t* eout, const int16_t* vb,
                         int64_t stride, const int32_t* eb, int64_t nchunks, const double* R scale,
                         const double* R adev, int nv, int64_t n, double* R partial, const int* R stop) {
  cgs_maxpy_norm<B16>(WPlain{win}, B16::Out{cur, vout, eout}, B16::Basis{vb, stride, eb, nchunks}, scale, adev, nv, n,
                      partial, stop);
}
KERNEL k_cb16_accum(double* R x, const int* R nvdev, const int16_t* R vb, int64_t stride, const int32_t* R eb,
                    int64_t nchunks, const double* R scale, const double* R coef, int64_t n, const int* R stop) {
  cgs_accum<B16>(x, nvdev, B16::Basis{vb, stride, eb, nchunks}, scale, coef, n, stop);
}

KERNEL k_pcj_apply_norm(const double* r, const double* R dinv, double* z, int64_t n, double* R partial,
                        const int* R stop) {
  cgs_store<F64>(WDinv{r, dinv}, F64::Out{z}, n, partial, stop);
}
KERNEL k_pcj_mdot(const double* R w, const double* R dinv, const double* R vb, int64_t stride, const double* R scale,
                  int nv, int64_t n, double* R partial, int64_t nchunks, const int* R stop) {
  cgs_mdot<F64>(WDinv{w, dinv}, F64::Basis{vb, stride}, scale, nv, n, partial, nchunks, stop);
}
KERNEL k_pcj_maxpy_norm(const double* R win, const double* R dinv, double* vout, const double* vb, int64_t stride,
                        const double* R scale, const double* R adev, int nv, int64_t n, double* R partial,
                        const int* R stop) {
  cgs_maxpy_norm<F64>(WDinv{win, dinv}, F64::Out{vout}, F64::Basis{vb, stride}, scale, adev, nv, n, partial, stop);
}

#undef R
#undef KERNEL

inline int nchunks32(int64_t n) { return (int)((n + kChunk - 1) / kChunk); }

}  // namespace

// one workgroup per chunk of n
#define LAUNCH(kernel, n, s, ...) \
  (kernel<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(__VA_ARGS__), (int)hipGetLastError())

extern "C" int msk_cb_round_store(const double* r, double* cur, float* v0, int64_t n, double* partial, const int* stop,
                                  hipStream_t s) {
  return LAUNCH(k_cb_round_store, n, s, r, cur, v0, n, partial, stop);
}

extern "C" int msk_cb_mdot(const double* w, const float* vb, int64_t stride, const double* scale, int nv, int64_t n,
                           double* partial, int64_t nchunks, const int* stop, hipStream_t s) {
  if (nv < 1 || nv > MSK_CB_MAX_GROUP) return (int)hipErrorInvalidValue;
  return LAUNCH(k_cb_mdot, n, s, w, vb, stride, scale, nv, n, partial, nchunks, stop);
}

extern "C" int msk_cb_maxpy_norm(const double* win, double* cur, float* vout, const float* vb, int64_t stride,
                                 const double* scale, const double* adev, int nv, int64_t n, double* partial,
                                 const int* stop, hipStream_t s) {
  return LAUNCH(k_cb_maxpy_norm, n, s, win, cur, vout, vb, stride, scale, adev, nv, n, partial, stop);
}

extern "C" int msk_cb_accum(double* x, const int* nvdev, const float* vb, int64_t stride, const double* scale,
                            const double* coef, int64_t n, const int* stop, hipStream_t s) {
  return LAUNCH(k_cb_accum, n, s, x, nvdev, vb, stride, scale, coef, n, stop);
}

extern "C" int msk_cb16_round_store(const double* r, double* cur, int16_t* v0, int32_t* e0, int64_t n,
                                    double* partial, const int* stop, hipStream_t s) {
  return LAUNCH(k_cb16_round_store, n, s, r, cur, v0, e0, n, partial, stop);
}

extern "C" int msk_cb16_mdot(const double* w, const int16_t* vb, int64_t stride, const int32_t* eb,
                             const double* scale, int nv, int64_t n, double* partial, int64_t nchunks,
                             const int* stop, hipStream_t s) {
  if (nv < 1 || nv > MSK_CB_MAX_GROUP || nchunks != nchunks32(n)) return (int)hipErrorInvalidValue;
  return LAUNCH(k_cb16_mdot, n, s, w, vb, stride, eb, scale, nv, n, partial, nchunks, stop);
}

extern "C" int msk_cb16_maxpy_norm(const double* win, double* cur, int16_t* vout, int32_t* eout, const int16_t* vb,
                                   int64_t stride, const int32_t* eb, const double* scale, const double* adev,
                                   int nv, int64_t n, double* partial, const int* stop, hipStream_t s) {
  return LAUNCH(k_cb16_maxpy_norm, n, s, win, cur, vout, eout, vb, stride, eb, nchunks32(n), scale, adev, nv, n,
                partial, stop);
}

extern "C" int msk_cb16_accum(double* x, const int* nvdev, const int16_t* vb, int64_t stride, const int32_t* eb,
                              const double* scale, const double* coef, int64_t n, const int* stop, hipStream_t s) {
  return LAUNCH(k_cb16_accum, n, s, x, nvdev, vb, stride, eb, nchunks32(n), scale, coef, n, stop);
}

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
  return LAUNCH(k_pcj_apply_norm, n, s, r, dinv, z, n, partial, stop);
}

extern "C" int msk_pcj_mdot(const double* w, const double* dinv, const double* vb, int64_t stride,
                            const double* scale, int nv, int64_t n, double* partial, int64_t nchunks,
                            const int* stop, hipStream_t s) {
  if (nv < 1 || nv > MSK_CB_MAX_GROUP || nchunks != nchunks32(n)) return (int)hipErrorInvalidValue;
  return LAUNCH(k_pcj_mdot, n, s, w, dinv, vb, stride, scale, nv, n, partial, nchunks, stop);
}

extern "C" int msk_pcj_maxpy_norm(const double* win, const double* dinv, double* vout, const double* vb,
                                  int64_t stride, const double* scale, const double* adev, int nv, int64_t n,
                                  double* partial, const int* stop, hipStream_t s) {
  if (nv < 1) return (int)hipErrorInvalidValue;
  return LAUNCH(k_pcj_maxpy_norm, n, s, win, dinv, vout, vb, stride, scale, adev, nv, n, partial, stop);
}

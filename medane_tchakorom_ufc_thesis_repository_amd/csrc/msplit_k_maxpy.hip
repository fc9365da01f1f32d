// msplit_k_maxpy.hip -- the vector-major VecMAXPY of the GMRES inner-solve path: k_maxpy_chunk and k_maxpy_op
// (W = A (sc x) computed in the kernel), with their launchers msk_maxpy_chunk and msk_maxpy_op.
#include "msplit_kdev.hpp"

namespace msk {
namespace {  // internal linkage: a unit's kernels are launched from this unit only

// ------------------------------------------------------------------ MAXPY
// Vector-major MAXPY in the DBR chunk layout: workgroup c owns elements
// [4096c, 4096c+4096); lane t owns base + j*512 + 2t, +1 (j = 0..7) and keeps
// their 16 running values in registers while the vectors stream past group by
// group (each group = up to 4 vectors x 32 KiB contiguous per workgroup).
// Per element the arithmetic is PETSc VecMAXPY_Seq's: the nv&3 leading vectors
// (PetscKernelAXPY3/2/1), then groups of four (PetscKernelAXPY4),
// U += a0*p0 + a1*p1 + a2*p2 + a3*p3 evaluated left to right.
// NORM: also the DBR partial of ||w_new||^2 for this chunk (VecNorm fused).
template <int G, bool FULL, int VAR, int J0, int JN>
__device__ __forceinline__ void chunk_group(double (&u)[2 * kIters], const Vecs& V, const Coefs& A,
                                            const double* __restrict__ adev, int negate, int g, int64_t base,
                                            int64_t n) {
  double a[G], sv[G];
  const double* vp[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {  // wave-uniform: scalar loads from the kernel arguments / adev
    const double aq = adev ? adev[g + q] : A.a[g + q];
    a[q] = negate ? -aq : aq;
    vp[q] = vec_at(V, g + q);
    sv[q] = vec_scale(V, g + q);
  }
#pragma unroll
  for (int j = J0; j < J0 + JN; ++j) {
    const int64_t e = base + j * (2 * kT);
    double p0[G], p1[G];
#pragma unroll
    for (int q = 0; q < G; ++q) {
      if (FULL) {
        const double2* pv = reinterpret_cast<const double2*>(vp[q] + e);
        const double2 v = (VAR & 1) ? ld_nt(pv) : *pv;
        p0[q] = v.x * sv[q];
        p1[q] = v.y * sv[q];
      } else {
        p0[q] = e < n ? vp[q][e] * sv[q] : 0.0;
        p1[q] = e + 1 < n ? vp[q][e + 1] * sv[q] : 0.0;
      }
    }
    const double s0 = group_sum<G>(a, p0), s1 = group_sum<G>(a, p1);
    if constexpr (G == 1) {  // PetscKernelAXPY: s = a*p; s += U
      u[2 * j] = s0 + u[2 * j];
      u[2 * j + 1] = s1 + u[2 * j + 1];
    } else {
      u[2 * j] = u[2 * j] + s0;
      u[2 * j + 1] = u[2 * j + 1] + s1;
    }
  }
}

// One slice [J0, J0+JN) of the lane's 8 double2 positions: load w, run every
// vector group over it, store and add its squares to acc in j order.  The
// chunk is one slice (VAR bit 3 clear) or two halves one after the other (set:
// half the registers, twice the waves per SIMD); per element nothing changes.
template <bool ACCUM, bool NORM, bool FULL, int VAR, int J0, int JN, bool OPW = false>
__device__ __forceinline__ void maxpy_slice(const double* __restrict__ win, double* __restrict__ wout,
                                            const Vecs& V, const Coefs& A, const double* __restrict__ adev,
                                            int negate, int nv, int64_t base, int64_t n, double& acc,
                                            const EllOp* op = nullptr, const int32_t* sdel = nullptr,
                                            const double* sval = nullptr) {
  double u[2 * kIters];
  if constexpr (OPW) {
    ell_rows<J0, JN>(*op, sdel, sval, *op->sdev, base, n, u);
  } else {
#pragma unroll
    for (int j = J0; j < J0 + JN; ++j) {
      const int64_t e = base + j * (2 * kT);
      if (ACCUM) {
        u[2 * j] = 0.0;
        u[2 * j + 1] = 0.0;
      } else if (FULL) {
        const double2 q = *reinterpret_cast<const double2*>(win + e);
        u[2 * j] = q.x;
        u[2 * j + 1] = q.y;
      } else {
        u[2 * j] = e < n ? win[e] : 0.0;
        u[2 * j + 1] = e + 1 < n ? win[e + 1] : 0.0;
      }
    }
  }
  const int jrem = nv & 3;
  if (jrem == 3) chunk_group<3, FULL, VAR, J0, JN>(u, V, A, adev, negate, 0, base, n);
  else if (jrem == 2) chunk_group<2, FULL, VAR, J0, JN>(u, V, A, adev, negate, 0, base, n);
  else if (jrem == 1) chunk_group<1, FULL, VAR, J0, JN>(u, V, A, adev, negate, 0, base, n);
  if constexpr ((VAR & 32) != 0) {  // two groups per iteration: the compiler issues 8 vectors' loads at once
#pragma unroll 2
    for (int g = jrem; g < nv; g += 4) chunk_group<4, FULL, VAR, J0, JN>(u, V, A, adev, negate, g, base, n);
  } else {
#pragma unroll 1
    for (int g = jrem; g < nv; g += 4) chunk_group<4, FULL, VAR, J0, JN>(u, V, A, adev, negate, g, base, n);
  }
#pragma unroll
  for (int j = J0; j < J0 + JN; ++j) {
    const int64_t e = base + j * (2 * kT);
    double r0 = u[2 * j], r1 = u[2 * j + 1];
    if (FULL) {
      if (ACCUM) {  // VecAXPY(x, 1.0, T): x + T
        const double2 q = *reinterpret_cast<const double2*>(win + e);
        r0 = q.x + r0;
        r1 = q.y + r1;
      }
      if constexpr ((VAR & 4) != 0) {
        dx2 o;
        o.x = r0;
        o.y = r1;
        __builtin_nontemporal_store(o, reinterpret_cast<dx2*>(wout + e));
      } else {
        *reinterpret_cast<double2*>(wout + e) = make_double2(r0, r1);
      }
      if (NORM) {
        acc = acc + r0 * r0;
        acc = acc + r1 * r1;
      }
    } else {
      if (e < n) {
        if (ACCUM) r0 = win[e] + r0;
        wout[e] = r0;
        if (NORM) acc = acc + r0 * r0;
      }
      if (e + 1 < n) {
        if (ACCUM) r1 = win[e + 1] + r1;
        wout[e + 1] = r1;
        if (NORM) acc = acc + r1 * r1;
      }
    }
  }
}

template <bool ACCUM, bool NORM, bool FULL, int VAR, bool OPW = false>
__device__ __forceinline__ void maxpy_chunk_body(const double* __restrict__ win, double* __restrict__ wout,
                                                 const Vecs& V, const Coefs& A, const double* __restrict__ adev,
                                                 int negate, int nv, int64_t base, int64_t n, double& sq,
                                                 const EllOp* op = nullptr, const int32_t* sdel = nullptr,
                                                 const double* sval = nullptr) {
  double acc = 0.0;
  if constexpr ((VAR & 8) != 0) {
    maxpy_slice<ACCUM, NORM, FULL, VAR, 0, kIters / 2, OPW>(win, wout, V, A, adev, negate, nv, base, n, acc, op,
                                                            sdel, sval);
    maxpy_slice<ACCUM, NORM, FULL, VAR, kIters / 2, kIters / 2, OPW>(win, wout, V, A, adev, negate, nv, base, n,
                                                                     acc, op, sdel, sval);
  } else {
    maxpy_slice<ACCUM, NORM, FULL, VAR, 0, kIters, OPW>(win, wout, V, A, adev, negate, nv, base, n, acc, op, sdel,
                                                        sval);
  }
  sq = acc;
}

template <bool ACCUM, bool NORM, int VAR>
__global__ __launch_bounds__(kT) void k_maxpy_chunk(const double* win, double* wout, Vecs V, Coefs A,
                                                    const double* __restrict__ adev, int negate, int nv,
                                                    const int* __restrict__ nvdev, int64_t n,
                                                    double* __restrict__ partial, const int* __restrict__ stop) {
  if (stopped(stop)) return;
  if (nvdev) nv = *nvdev;
  if (nv <= 0) return;
  const int t = threadIdx.x;
  const int64_t c = (VAR & 64) ? (int64_t)gridDim.x - 1 - blockIdx.x : blockIdx.x;  // 64: top chunks first
  const int64_t base = c * kChunk + 2 * t;
  double sq = 0.0;
  if ((c + 1) * kChunk <= n) maxpy_chunk_body<ACCUM, NORM, true, VAR>(win, wout, V, A, adev, negate, nv, base, n, sq);
  else maxpy_chunk_body<ACCUM, NORM, false, VAR>(win, wout, V, A, adev, negate, nv, base, n, sq);
  if (NORM) {
    __shared__ double red[4];
    sq = wave_butterfly(sq);
    if ((t & 63) == 0) red[t >> 6] = sq;
    __syncthreads();
    if (t == 0) partial[c] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// CGS VecMAXPY with W = A (sc x) computed in the kernel, and the ||w||^2 partials.
template <int VAR>
__global__ __launch_bounds__(kT) void k_maxpy_op(EllOp op, double* wout, Vecs V, const double* __restrict__ adev,
                                                 int nv, int64_t n, double* __restrict__ partial,
                                                 const int* __restrict__ stop) {
  __shared__ int32_t sdel[kT];
  __shared__ double sval[kT];
  __shared__ double red[4];
  ell_dict_stage(op, sdel, sval);
  if (stopped(stop)) return;  // uniform
  __syncthreads();
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x;
  const int64_t base = c * kChunk + 2 * t;
  const Coefs A = {};
  double sq = 0.0;
  if ((c + 1) * kChunk <= n)
    maxpy_chunk_body<false, true, true, VAR, true>(nullptr, wout, V, A, adev, 1, nv, base, n, sq, &op, sdel, sval);
  else
    maxpy_chunk_body<false, true, false, VAR, true>(nullptr, wout, V, A, adev, 1, nv, base, n, sq, &op, sdel, sval);
  sq = wave_butterfly(sq);
  if ((t & 63) == 0) red[t >> 6] = sq;
  __syncthreads();
  if (t == 0) partial[c] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace
}  // namespace msk

// ===================================================================== launchers
using namespace msk;

// The bits of the MAXPY kernels' VAR.  VAR is a template argument and so part of every kernel's name: the values stay.
enum { kVarNtLoad = 1, kVarNtStore = 4, kVarHalves = 8, kVarUnroll2 = 32, kVarTopFirst = 64 };

extern "C" int msk_maxpy_op(const EllOp* op, double* wout, const Vecs* V, int nv, const double* adev, int64_t n,
                            double* partial, const int* stop, hipStream_t s) {
  if (n <= 0 || nv <= 0) return 0;
  if (op->ndict > 255) return (int)hipErrorInvalidValue;
  const unsigned g = (unsigned)((n + kChunk - 1) / kChunk);
  const int var = vec_var() | ((msk_tuning_flags & MSK_TUNE_MAXPY_TEMPORAL_ST) ? 0 : kVarNtStore);
  pick<5, 4, 1, 0>(var, [&](auto v) {
    k_maxpy_op<decltype(v)::value><<<g, kT, 0, s>>>(*op, wout, *V, adev, nv, n, partial, stop);
  });
  return (int)hipGetLastError();
}

extern "C" int msk_maxpy_chunk(const double* win, double* wout, const Vecs* V, int nv, const int* nvdev,
                               const Coefs* A, const double* adev, int negate, int64_t n, int accum, double* partial,
                               const int* stop, hipStream_t s) {
  if (n <= 0 || (nv <= 0 && !nvdev)) return 0;
  // non-temporal store of w too unless MSK_TUNE_MAXPY_TEMPORAL_ST (+0.4 % per step); the group loop
  // unrolled by two unless MSK_TUNE_MAXPY_UNROLL1 (+1.7 % per step: 64-load bursts at one wave per SIMD)
  int var = vec_var() | ((msk_tuning_flags & MSK_TUNE_MAXPY_TEMPORAL_ST) ? 0 : kVarNtStore) |
            ((msk_tuning_flags & MSK_TUNE_MAXPY_HALVES) ? kVarHalves : 0) |
            ((msk_tuning_flags & MSK_TUNE_MAXPY_UNROLL1) ? 0 : kVarUnroll2);
  // Top chunk first where a vector outgrows the 256 MiB MALL (n > 2^25): MAXPY then starts on the rows the
  // fused MatMult+MDot (or the MDot) left in the MALL and ends on those the next one starts with (SMSM's
  // 512x512x256 block +1.0 %, MAXPY 5.68 -> 5.86 TB/s; at 256^3, where whole vectors fit, -0.7 %; same box,
  // profiles/r03/rev_ab/).  MSPLIT_MAXPY_REV=0/1 forces either order (maxpy_rev).  Only the two variants with
  // non-temporal loads and the unrolled group loop (33, 37) have the reversed form (97, 101).
  if (maxpy_rev(n) && (var == 33 || var == 37)) var |= kVarTopFirst;
  const unsigned g = (unsigned)((n + kChunk - 1) / kChunk);
  const bool known = pick<0, 1, 4, 5, 13, 32, 33, 36, 37, 45, 97, 101>(var, [&](auto v) {
    constexpr int VAR = decltype(v)::value;
    if (partial)  // with the ||w||^2 partials
      k_maxpy_chunk<false, true, VAR><<<dim3(g), dim3(kT), 0, s>>>(win, wout, *V, *A, adev, negate, nv, nvdev, n, partial,
                                                                   stop);
    else
      pick<true, false>(accum != 0, [&](auto acc) {
        k_maxpy_chunk<decltype(acc)::value, false, VAR><<<dim3(g), dim3(kT), 0, s>>>(win, wout, *V, *A, adev, negate, nv,
                                                                                   nvdev, n, partial, stop);
      });
  });
  if (!known) return (int)hipErrorInvalidValue;  // a tuning combination with no kernel: fail, never run another one
  return (int)hipGetLastError();
}

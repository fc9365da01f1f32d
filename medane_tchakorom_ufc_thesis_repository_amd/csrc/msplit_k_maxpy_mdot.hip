// msplit_k_maxpy_mdot.hip -- the first CGS pass fused with the second pass' VecMDot (GMRES with
// -ksp_gmres_cgs_refinement_type refine_ifneeded / refine_always): k_maxpy_mdot and its launcher msk_maxpy_mdot.
//
// One sweep over the basis computes u = W - sum_j h_j v_j (k_maxpy_chunk's arithmetic), stores it, and leaves the
// DBR stage-1 partials of ||u||^2 and of every c_j = u . v_j (dot_chunk's arithmetic): MAXPY and MDot stage 1 use
// the same lane map, lane t of chunk c owns base + j*512 + 2t, +1 (j = 0..7), so the u a lane has just formed is the
// w that the MDot would have re-read, and p = v * sc is the value both multiply.  The kernels it replaces stream
// the basis twice (nv + 2 and nv + 1 vectors); this one streams it once.
#include "msplit_kdev.hpp"

namespace msk {
namespace {  // internal linkage: a unit's kernels are launched from this unit only

// JU slices (double2 positions j) of the lane at a time: the NV x JU basis loads are issued before the first
// product, about 128 VGPRs of loads in flight whatever NV is (one wave per SIMD, k_lsqr_onepass's regime).
template <int NV>
constexpr int slices_at_once() {
  return NV <= 4 ? 8 : NV <= 8 ? 4 : NV <= 16 ? 2 : 1;
}

// One element's pass-1 value in PETSc VecMAXPY_Seq's order (chunk_group): the NV & 3 leading vectors, then
// groups of four, each group's sum evaluated left to right.  a[q] = -h[q], p[q] = v_q * sc_q.
template <int NV>
__device__ __forceinline__ double maxpy_elem(double u, const double (&a)[NV], const double (&p)[NV]) {
  constexpr int R = NV & 3;
  if constexpr (R == 1) u = a[0] * p[0] + u;  // PetscKernelAXPY: s = a*p; s += U
  if constexpr (R == 2) u = u + (a[0] * p[0] + a[1] * p[1]);
  if constexpr (R == 3) u = u + ((a[0] * p[0] + a[1] * p[1]) + a[2] * p[2]);
#pragma unroll
  for (int g = R; g < NV; g += 4) {
    double s = a[g] * p[g] + a[g + 1] * p[g + 1];
    s = s + a[g + 2] * p[g + 2];
    s = s + a[g + 3] * p[g + 3];
    u = u + s;
  }
  return u;
}

// VAR: bit 0 = non-temporal loads of the basis, bit 2 = non-temporal store of u (k_maxpy_chunk's bits).
template <int NV, int VAR>
__global__ __launch_bounds__(kT) void k_maxpy_mdot(const double* __restrict__ win, double* __restrict__ wout, Vecs V,
                                                   const double* __restrict__ adev, int64_t n,
                                                   double* __restrict__ partial, int64_t nchunks, int rev,
                                                   const int* __restrict__ stop) {
  if (stopped(stop)) return;
  __shared__ double red[NV + 1][4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t c = rev ? (int64_t)gridDim.x - 1 - blockIdx.x : blockIdx.x;  // k_maxpy_chunk's top-chunks-first order
  const int64_t base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double a[NV], sv[NV];
  const double* vp[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) {  // wave-uniform
    a[q] = -adev[q];
    vp[q] = vec_at(V, q);
    sv[q] = vec_scale(V, q);
  }
  double acc[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) acc[q] = 0.0;
  double sq = 0.0;
  constexpr int JU = slices_at_once<NV>();
  if (full) {
#pragma unroll 1
    for (int j0 = 0; j0 < kIters; j0 += JU) {
      double2 v[JU][NV], w[JU];
#pragma unroll
      for (int jj = 0; jj < JU; ++jj) {
        const int64_t e = base + (j0 + jj) * (2 * kT);
        w[jj] = *reinterpret_cast<const double2*>(win + e);
#pragma unroll
        for (int q = 0; q < NV; ++q) {
          const double2* pv = reinterpret_cast<const double2*>(vp[q] + e);
          v[jj][q] = (VAR & 1) ? ld_nt(pv) : *pv;
        }
      }
#pragma unroll
      for (int jj = 0; jj < JU; ++jj) {
        const int64_t e = base + (j0 + jj) * (2 * kT);
        double p0[NV], p1[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) {
          p0[q] = v[jj][q].x * sv[q];
          p1[q] = v[jj][q].y * sv[q];
        }
        const double r0 = maxpy_elem<NV>(w[jj].x, a, p0), r1 = maxpy_elem<NV>(w[jj].y, a, p1);
        if constexpr ((VAR & 4) != 0) {
          dx2 o;
          o.x = r0;
          o.y = r1;
          __builtin_nontemporal_store(o, reinterpret_cast<dx2*>(wout + e));
        } else {
          *reinterpret_cast<double2*>(wout + e) = make_double2(r0, r1);
        }
        sq = sq + r0 * r0;
        sq = sq + r1 * r1;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
          acc[q] = acc[q] + r0 * p0[q];
          acc[q] = acc[q] + r1 * p1[q];
        }
      }
    }
  } else {  // the ragged last chunk: every access guarded, absent elements add nothing (dot_chunk's guards)
#pragma unroll 1
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      const bool in0 = e < n, in1 = e + 1 < n;
      double p0[NV], p1[NV];
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        p0[q] = in0 ? vp[q][e] * sv[q] : 0.0;
        p1[q] = in1 ? vp[q][e + 1] * sv[q] : 0.0;
      }
      const double r0 = maxpy_elem<NV>(in0 ? win[e] : 0.0, a, p0);
      const double r1 = maxpy_elem<NV>(in1 ? win[e + 1] : 0.0, a, p1);
      if (in0) {
        wout[e] = r0;
        sq = sq + r0 * r0;
      }
      if (in1) {
        wout[e + 1] = r1;
        sq = sq + r1 * r1;
      }
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        if (in0) acc[q] = acc[q] + r0 * p0[q];
        if (in1) acc[q] = acc[q] + r1 * p1[q];
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const double s = wave_butterfly(acc[q]);
    if (lane == 0) red[q][wv] = s;
  }
  sq = wave_butterfly(sq);
  if (lane == 0) red[NV][wv] = sq;
  __syncthreads();
  if (t <= NV) partial[t * nchunks + c] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
}

}  // namespace
}  // namespace msk

// ===================================================================== launcher
using namespace msk;

extern "C" int msk_maxpy_mdot(const double* win, double* wout, const Vecs* V, int nv, const double* adev, int64_t n,
                              double* partial, int64_t nchunks, const int* stop, hipStream_t s) {
  if (n <= 0 || nchunks <= 0) return 0;
  if (nv < 1 || nv + 1 > MSK_MAX_GROUP) return (int)hipErrorInvalidValue;  // partial has MSK_MAX_GROUP rows
  const int rev = maxpy_rev(n);  // msk_maxpy_chunk's order
  // the store policy follows MSK_TUNE_MAXPY_TEMPORAL_ST; the basis loads are non-temporal
  pick<1, 5>((msk_tuning_flags & MSK_TUNE_MAXPY_TEMPORAL_ST) ? 1 : 5, [&](auto var) {
    pick_range<1, MSK_MAX_GROUP - 1>(nv, [&](auto k) {
      k_maxpy_mdot<decltype(k)::value, decltype(var)::value><<<dim3((unsigned)nchunks), dim3(kT), 0, s>>>(
          win, wout, *V, adev, n, partial, nchunks, rev, stop);
    });
  });
  return (int)hipGetLastError();
}

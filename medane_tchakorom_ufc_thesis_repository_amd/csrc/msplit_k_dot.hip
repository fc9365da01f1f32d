// msplit_k_dot.hip -- the DBR dots (VecMDot, VecNorm) of the GMRES inner-solve path: k_dot_stage1 in its
// default variant and k_dot_stage2, with their launchers msk_dot_stage1 and msk_dot_stage2.  The chunk bodies
// (dot_chunk, dot_group_full) and k_dot_stage1 itself are in msplit_kdev.hpp; the A/B variants of stage 1 are
// msplit_k_dot_a.hip and _b.hip, and stage 1 with W computed in the kernel is msplit_k_dot_op.hip.
#include "msplit_kdev.hpp"

namespace msk {
namespace {  // internal linkage: a unit's kernels are launched from this unit only

// Stage 2: workgroup v folds the nchunks partials of vector v the same way.
template <bool HS>
__global__ __launch_bounds__(kT) void k_dot_stage2(const double* __restrict__ partial, int64_t nchunks,
                                                   double* __restrict__ out, const int* __restrict__ stop) {
  // the stop flag (HS: stop is not null) is read together with the partials and tested after the
  // (convergent) butterfly, so a running cycle waits for one round of loads, not two
  bool skip = false;
  if constexpr (HS) skip = *stop != 0;
  __shared__ double red[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const double* p = partial + blockIdx.x * nchunks;
  double acc = 0.0;
  int64_t i = t;
  // 16, then 8 loads in flight per lane, added in the same order (lane t: p[t], p[t+256], ...)
  for (; i + 15 * kT < nchunks; i += 16 * kT) {
    double q[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) q[u] = p[i + u * kT];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc = acc + q[u];
  }
  for (; i + 7 * kT < nchunks; i += 8 * kT) {
    double q[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) q[u] = p[i + u * kT];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = acc + q[u];
  }
  for (; i < nchunks; i += kT) acc = acc + p[i];
  acc = wave_butterfly(acc);
  if (skip) return;  // uniform
  if (lane == 0) red[wv] = acc;
  __syncthreads();
  if (t == 0) out[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace
}  // namespace msk

// ===================================================================== launchers
using namespace msk;

extern "C" int msk_dot_stage1(const double* w, const Vecs* V, int nv, int64_t n, double* partial, int64_t nchunks,
                              int self, const int* stop, hipStream_t s) {
  if (nchunks <= 0) return 0;
  if (!self && (nv < 1 || nv > MSK_MAX_GROUP)) return (int)hipErrorInvalidValue;
  const int var = vec_var() | ((msk_tuning_flags & MSK_TUNE_MDOT_SINGLE) ? 16 : 0) |
                  ((msk_tuning_flags & MSK_TUNE_MDOT_UNROLL2) ? 32 : 0);
  if (self)
    k_dot_stage1<1, true, 0><<<dim3((unsigned)nchunks), dim3(kT), 0, s>>>(w, *V, n, partial, nchunks, stop, 0);
  else if (var == 1) dot1_launch<1>(nv, w, *V, n, partial, nchunks, stop, s);
  else if (msk_dot1_variants_a(var, nv, w, *V, n, partial, nchunks, stop, s) &&
           msk_dot1_variants_b(var, nv, w, *V, n, partial, nchunks, stop, s))
    return (int)hipErrorInvalidValue;  // a tuning combination with no kernel: fail, never run another one
  return (int)hipGetLastError();
}

extern "C" int msk_dot_stage2(const double* partial, int64_t nchunks, int nv, double* out, const int* stop,
                              hipStream_t s) {
  pick<true, false>(stop != nullptr, [&](auto hs) {
    k_dot_stage2<decltype(hs)::value><<<dim3(nv), dim3(kT), 0, s>>>(partial, nchunks, out, stop);
  });
  return (int)hipGetLastError();
}

// msplit_k_dot_op.hip -- MDot stage 1 with W = A (sc x) computed in the kernel (k_dot_stage1_op, the DV
// operator in ELL layout) and its launcher msk_dot_stage1_op, in an object of its own: 64 instantiations, which
// build beside the other dot units.  The chunk body (dot_chunk with ell_rows) is in msplit_kdev.hpp.
#include "msplit_kdev.hpp"

namespace msk {
namespace {  // internal linkage: a unit's kernels are launched from this unit only

// Stage 1 with W = A (sc x) computed in the kernel (no W vector in HBM).
template <int NV, int VAR>
__global__ __launch_bounds__(kT) void k_dot_stage1_op(EllOp op, Vecs V, int64_t n, double* __restrict__ partial,
                                                      int64_t nchunks, const int* __restrict__ stop) {
  __shared__ double red[NV][4];
  __shared__ int32_t sdel[kT];
  __shared__ double sval[kT];
  ell_dict_stage(op, sdel, sval);
  if (stopped(stop)) return;  // uniform: every lane reads the same flag
  __syncthreads();
  dot_chunk<NV, false, VAR, true>(nullptr, V, n, partial, nchunks, 0, blockIdx.x, red, &op, sdel, sval);
}

}  // namespace
}  // namespace msk

// ===================================================================== launchers
using namespace msk;

extern "C" int msk_dot_stage1_op(const EllOp* op, const Vecs* V, int nv, int64_t n, double* partial,
                                 int64_t nchunks, const int* stop, hipStream_t s) {
  if (nchunks <= 0) return 0;
  if (nv < 1 || nv > MSK_MAX_GROUP || op->ndict > 255) return (int)hipErrorInvalidValue;
  pick<1, 0>(vec_var(), [&](auto var) {
    pick_range<1, MSK_MAX_GROUP>(nv, [&](auto k) {
      k_dot_stage1_op<decltype(k)::value, decltype(var)::value><<<dim3((unsigned)nchunks), dim3(kT), 0, s>>>(
          *op, *V, n, partial, nchunks, stop);
    });
  });
  return (int)hipGetLastError();
}

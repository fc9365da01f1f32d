// msplit_k_dot_b.hip -- A/B variants of the MDot stage-1 kernel (k_dot_stage1, msplit_kdev.hpp) for
// msk_dot_stage1 (msplit_k_dot.hip), in an object of their own: each variant is 32 instantiations, and the two
// objects build beside each other.
#include "msplit_kdev.hpp"

using namespace msk;

// Returns 0 when it launched the variant, 1 when the variant is not one of these.
int msk_dot1_variants_b(int var, int nv, const double* w, const Vecs& V, int64_t n, double* partial,
                        int64_t nchunks, const int* stop, hipStream_t s) {
  return pick<17, 32, 33>(var, [&](auto v) { dot1_launch<decltype(v)::value>(nv, w, V, n, partial, nchunks, stop, s); })
             ? 0
             : 1;
}

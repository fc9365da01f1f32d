// msplit_k_diffusion.hip -- device assembly of the variable-coefficient diffusion operator -div(kappa grad u) on a
// box (msp_mat_create_box_diffusion): the hashed test field, the CSR from a coefficient vector, and the STENCIL
// storage (msplit_runtime.hip rv_attach's layouts) built from that CSR without a host copy.
//
// Compiled with -ffp-contract=off like every unit: each *, + and / below rounds on its own, so the values are the
// bits numpy gives for the same expressions (utils.diffusion_rows, utils.heterogeneous_poisson3d).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "msplit_kernels.h"
#include "msplit_kdev.hpp"

namespace msk {
namespace {  // internal linkage: the kernels are launched from this file only

// kappa(c) = 1.0 + (double)(splitmix64(c + seed) mod 1000) * 0.001 for the cells first + i: 64-bit integer
// arithmetic (wrapping, as numpy's uint64), one exact u64 -> f64 conversion (< 1000), one multiply, one add.
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(kT) void k_cell_coefficients(double* __restrict__ kappa, int64_t n, uint64_t first,
                                                          uint64_t seed) {
  const int64_t stride = (int64_t)gridDim.x * kT;
  for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += stride) {
    const uint64_t h = splitmix64(first + (uint64_t)i + seed);
    const double m = (double)(h % 1000ull) * 0.001;
    kappa[i] = 1.0 + m;
  }
}

// The face weight between the row's cell (ka) and a neighbour cell (kb): ((2 ka) kb) / (ka + kb), numpy's
// left-to-right order of 2.0 * ka * kb / (ka + kb).
__device__ __forceinline__ double face_weight(double ka, double kb) { return ((2.0 * ka) * kb) / (ka + kb); }

// Rows of the diffusion operator from kappa = [ghost plane below if glo | the block's planes | ghost plane above
// if ghi] (P doubles per plane).  Row pointers in closed form (box_rowptr with k_box_stencil's lo / hi
// corrections); a lane reads kappa of its own cell and of the neighbours that exist -- inside the box, or in a
// ghost plane where the flag says there is one -- so nothing outside [0, (glo + ns + ghi) P) is read.  A face with
// no cell behind it weighs the cell's own kappa.  Columns as k_box_stencil: [plane below if lo | own | plane above
// if hi]; lo <= glo and hi <= ghi (the caller checks).
__global__ __launch_bounds__(kT) void k_box_diffusion(int dim, int32_t nx, int32_t ny, int32_t nz, int64_t nrows,
                                                      int glo, int ghi, int lo, int hi,
                                                      const double* __restrict__ kappa, int32_t* __restrict__ rowptr,
                                                      int32_t* __restrict__ col, double* __restrict__ val) {
  const int64_t stride = (int64_t)gridDim.x * kT;
  const int64_t P = dim == 3 ? (int64_t)nx * ny : (int64_t)nx;  // slab plane
  const int64_t ns = dim == 3 ? nz : ny;                           // planes in the block
  const int64_t off = lo ? P : 0;
  const int64_t goff = glo ? P : 0;
  for (int64_t l = (int64_t)blockIdx.x * kT + threadIdx.x; l <= nrows; l += stride) {
    int64_t p0 = box_rowptr(dim, l, nx, ny, nz);
    if (lo) p0 += min(l, P);
    if (hi) p0 += max((int64_t)0, l - (ns - 1) * P);
    rowptr[l] = (int32_t)p0;
    if (l == nrows) continue;
    const int32_t i = (int32_t)(l % nx);
    const int32_t j = (int32_t)((l / nx) % ny);
    const int64_t sl = l / P;  // slab-plane index (k in 3D, j in 2D)
    const int64_t g = l + goff;  // the row's cell in kappa
    const double ka = kappa[g];
    const bool hsm = sl > 0 || glo, hsp = sl < ns - 1 || ghi;  // a cell behind the slow faces
    const bool hym = dim == 3 && j > 0, hyp = dim == 3 && j < ny - 1;
    const bool hxm = i > 0, hxp = i < nx - 1;
    const double wsm = hsm ? face_weight(ka, kappa[g - P]) : ka;
    const double wxm = hxm ? face_weight(ka, kappa[g - 1]) : ka;
    const double wxp = hxp ? face_weight(ka, kappa[g + 1]) : ka;
    const double wsp = hsp ? face_weight(ka, kappa[g + P]) : ka;
    double d;
    double wym = 0.0, wyp = 0.0;
    if (dim == 3) {
      wym = hym ? face_weight(ka, kappa[g - nx]) : ka;
      wyp = hyp ? face_weight(ka, kappa[g + nx]) : ka;
      d = ((((wsm + wym) + wxm) + wxp) + wyp) + wsp;
    } else {
      d = ((wsm + wxm) + wxp) + wsp;
    }
    const int64_t e = l + off;
    int64_t p = p0;
    if (sl > 0 || lo) { col[p] = (int32_t)(e - P); val[p++] = -wsm; }
    if (hym) { col[p] = (int32_t)(e - nx); val[p++] = -wym; }
    if (hxm) { col[p] = (int32_t)(e - 1); val[p++] = -wxm; }
    col[p] = (int32_t)e; val[p++] = d;
    if (hxp) { col[p] = (int32_t)(e + 1); val[p++] = -wxp; }
    if (hyp) { col[p] = (int32_t)(e + nx); val[p++] = -wyp; }
    if (sl < ns - 1 || hi) { col[p] = (int32_t)(e + P); val[p++] = -wsp; }
  }
}

// Whether a square CSR is symmetric bit for bit: every off-diagonal entry A[r, c] is looked up in row c as A[c, r]
// and the two values' bits compared (rv_attach's test for the symmetric storage; rows of at most a stencil's
// length, so the lookup is a short scan).  *fail is set on a mismatch or a missing mirror.
__global__ __launch_bounds__(kT) void k_csr_sym_check(int32_t nrows, const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, const double* __restrict__ val,
                                                      int* __restrict__ fail) {
  const int32_t r = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (r >= nrows) return;
  bool bad = false;
  for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
    const int32_t c = col[k];
    if (c == r) continue;
    bool found = false;
    for (int32_t q = rowptr[c]; q < rowptr[c + 1]; ++q)
      if (col[q] == r) {
        found = true;
        bad = bad || __double_as_longlong(val[q]) != __double_as_longlong(val[k]);
      }
    bad = bad || !found;
  }
  if (bad) atomicOr(fail, 1);
}

// The STENCIL storage of the square 3D CSR of an nx x ny x nz box: row r's presence byte (bit e: an entry at
// neighbour e of (-P, -nx, -1, 0, +1, +nx, +P)) and its values in one of rv_attach's three layouts --
//   NLEG 7, BLOCKED false: rv[e * stride + r];
//   NLEG 7, BLOCKED true:  the seven legs of each 512-row slice of a DBR chunk next to each other;
//   NLEG 4, BLOCKED true:  the same with the diagonal and the three upper legs only (the symmetric storage);
// 0.0 where the row has no entry.  An entry whose column is no neighbour's sets *fail.
template <int NLEG, bool BLOCKED>
__global__ __launch_bounds__(kT) void k_csr_to_rv(int32_t nrows, int32_t nx, int32_t P, int64_t stride,
                                                  const int32_t* __restrict__ rowptr,
                                                  const int32_t* __restrict__ col, const double* __restrict__ val,
                                                  uint8_t* __restrict__ mask, double* __restrict__ rv,
                                                  int* __restrict__ fail) {
  const int32_t r = (int32_t)blockIdx.x * kT + (int32_t)threadIdx.x;
  if (r >= nrows) return;
  double leg[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  uint32_t m = 0;
  bool bad = false;
  for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
    const int32_t d = col[k] - r;
    const int e = d == -P ? 0 : d == -nx ? 1 : d == -1 ? 2 : d == 0 ? 3 : d == 1 ? 4 : d == nx ? 5 : d == P ? 6 : -1;
    if (e < 0) {
      bad = true;
      continue;
    }
    m |= 1u << e;
#pragma unroll
    for (int q = 0; q < 7; ++q)
      if (q == e) leg[q] = val[k];
  }
  if (bad) atomicOr(fail, 1);
  mask[r] = (uint8_t)m;
  if constexpr (BLOCKED) {
    const int64_t o = r % kChunk;
    const int64_t base = (int64_t)NLEG * (r - o) + (o / 512) * (NLEG * 512) + o % 512;
#pragma unroll
    for (int k = 0; k < NLEG; ++k) rv[base + k * 512] = leg[NLEG == 4 ? 3 + k : k];
  } else {
#pragma unroll
    for (int k = 0; k < 7; ++k) rv[(int64_t)k * stride + r] = leg[k];
  }
}

inline unsigned grid_rows(int64_t n, int64_t cap) {
  const int64_t g = (n + kT - 1) / kT;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace
}  // namespace msk

using namespace msk;

extern "C" int msk_cell_coefficients(double* kappa, int64_t n, uint64_t first, uint64_t seed, hipStream_t s) {
  if (n <= 0) return 0;
  k_cell_coefficients<<<dim3(grid_rows(n, 8192)), dim3(kT), 0, s>>>(kappa, n, first, seed);
  return (int)hipGetLastError();
}

extern "C" int msk_box_diffusion(int dim, int32_t nx, int32_t ny, int32_t nz, int64_t nrows, int glo, int ghi, int lo,
                                 int hi, const double* kappa, int32_t* rowptr, int32_t* col, double* val,
                                 hipStream_t s) {
  if (lo > glo || hi > ghi) return (int)hipErrorInvalidValue;
  k_box_diffusion<<<dim3(grid_rows(nrows + 1, 8192)), dim3(kT), 0, s>>>(dim, nx, ny, nz, nrows, glo, ghi, lo, hi, kappa,
                                                                         rowptr, col, val);
  return (int)hipGetLastError();
}

extern "C" int msk_csr_sym_check(int32_t nrows, const int32_t* rowptr, const int32_t* col, const double* val, int* fail,
                                 hipStream_t s) {
  if (nrows <= 0) return 0;
  k_csr_sym_check<<<(unsigned)(((int64_t)nrows + kT - 1) / kT), kT, 0, s>>>(nrows, rowptr, col, val, fail);
  return (int)hipGetLastError();
}

extern "C" int msk_csr_to_rv(int32_t nrows, int32_t nx, int32_t ny, int nleg, int blocked, int64_t stride,
                             const int32_t* rowptr, const int32_t* col, const double* val, uint8_t* mask, double* rv,
                             int* fail, hipStream_t s) {
  if (nrows <= 0) return 0;
  const int64_t P = (int64_t)nx * ny;
  if (nx <= 1 || ny <= 1 || P > INT32_MAX || (nleg != 4 && nleg != 7) || (nleg == 4 && !blocked) ||
      (blocked && nrows % MSK_DBR_CHUNK) || (!blocked && stride < nrows))
    return (int)hipErrorInvalidValue;
  const unsigned g = (unsigned)(((int64_t)nrows + kT - 1) / kT);
  const int form = nleg == 4 ? 2 : blocked ? 1 : 0;
  pick<0, 1, 2>(form, [&](auto f) {
    constexpr int F = decltype(f)::value;
    k_csr_to_rv<F == 2 ? 4 : 7, F != 0><<<g, kT, 0, s>>>(nrows, nx, (int32_t)P, stride, rowptr, col, val, mask, rv,
                                                        fail);
  });
  return (int)hipGetLastError();
}

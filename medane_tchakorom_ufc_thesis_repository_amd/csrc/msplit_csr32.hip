// msplit_csr32.hip -- the GMRES step's MatMult over a single-precision copy of a CSR operator's values
// (MSP_OPER_F32, msp_ksp_set_operator_precision), for gfx950.
//
// The copy holds one 8-byte word per stored entry, in CSR order: {int32 col, float val}, val = (float)a -- round to
// nearest even, gradual underflow, msplit_cgs_basis.hip's F32 conversion.  The f64 kernel k_spmv_lds8 streams 12
// bytes per entry (two arrays, two staging loops); this one streams 8 bytes in one loop.  All arithmetic stays f64:
//   s = s + (double)val_k * (x[col_k] * sc), entries in CSR order from 0.0, never contracted,
// which is k_spmv_lds8's SCALED sum statement for statement, so the product equals, bit for bit, the f64 kernel's
// product on a matrix whose values are (double)(float)a.  The row-block schedule (XcdMap) is the f64 kernel's: it
// changes no result, and it keeps a comparison of the two kernels one of bytes and not of order.
//
// The array holds nnz + 2 words and is 16-byte aligned: a row block's slice is staged from its first entry rounded
// down to an even one, in 16-byte transfers of two entries, so the last transfer can reach one entry beyond the
// block's end, and the block's end can be nnz.  k_csr32_pack writes the two slack words (column 0, value 0).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "msplit_kernels.h"
#include "msplit_kdev.hpp"

namespace msk {
namespace {

// ------------------------------------------------------------------------ pack
// One lane per entry.  A finite value whose float is not finite (|a| > FLT_MAX after rounding) is counted in
// *over (one vector atomic per such entry; the host reads the word once and refuses the copy); NaN and +-inf
// pass through as they are.
__global__ __launch_bounds__(kT) void k_csr32_pack(int64_t nnz, const int32_t* __restrict__ col,
                                                   const double* __restrict__ val, uint2* __restrict__ pk,
                                                   unsigned int* __restrict__ over) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= nnz + 2) return;
  uint2 e = make_uint2(0u, 0u);
  if (i < nnz) {
    const double a = val[i];
    const float f = (float)a;
    if (__builtin_isfinite(a) && !__builtin_isfinite(f)) atomicAdd(over, 1u);
    e.x = (uint32_t)col[i];
    e.y = __float_as_uint(f);
  }
  pk[i] = e;
}

// ---------------------------------------------------------------------- MatMult
// y = A~ (sc x), sc = *sdev.  k_spmv_lds8's shape: workgroup b owns rows [256b', 256b'+256) (b' by the schedule),
// one lane per row.  The block's packed slice goes to LDS by LDS-DMA in one loop: each wave instruction writes 64
// consecutive 16-byte slices; the tail lanes of the last instruction re-read the last slice into slack LDS, so the
// LDS capacity is rounded up to 256 entries (msk_spmv_p32).  The barrier waits for vmcnt(0).  Then per chunk of 8
// entries the 8 LDS reads and 8 x-gathers are issued before the first product, indices clamped to the row.  The
// packed stream is loaded non-temporally and y stored non-temporally (k_spmv_lds8's POL 3): neither should displace
// x from L2/MALL.
__global__ __launch_bounds__(kT) void k_spmv_p32(int32_t nrows, const int32_t* __restrict__ rowptr,
                                                 const uint2* __restrict__ pk, const double* __restrict__ x,
                                                 double* __restrict__ y, const double* __restrict__ sdev,
                                                 const int* __restrict__ stop, XcdMap xm) {
  if (stopped(stop)) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint2* sp = reinterpret_cast<const uint2*>(smem);
  const int t = threadIdx.x;
  const int32_t r0 = row_block(xm) * kT;
  const int32_t r1 = min(r0 + kT, nrows);
  const int32_t start = rowptr[r0], end = rowptr[r1];
  const int32_t s2 = start & ~1;
  const int32_t n2 = (end - s2 + 1) >> 1;  // 16-byte slices: entries [s2, s2 + 2 n2), at most one beyond end
  const uint4* p2 = reinterpret_cast<const uint4*>(pk + s2);
  const int32_t r = r0 + t;
  const double sc = *sdev;
  int32_t k0 = 0, k1 = 0;
  if (r < r1) {
    k0 = rowptr[r];
    k1 = rowptr[r + 1];
  }
  {
    const int lane = t & 63, w = t >> 6;
    for (int32_t ib = w * 64; ib < n2; ib += kT) glds16<true>(p2 + min(ib + lane, n2 - 1), smem + (size_t)ib * 16);
  }
  __syncthreads();
  if (r < r1) {
    double s = 0.0;
    for (int32_t kb = k0; kb < k1; kb += 8) {
      uint32_t av[8];
      double xv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const uint2 e = sp[min(kb + q, k1 - 1) - s2];
        av[q] = e.y;
        xv[q] = x[(int32_t)e.x];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        xv[q] = xv[q] * sc;
        if (kb + q < k1) s = s + (double)__uint_as_float(av[q]) * xv[q];
      }
    }
    __builtin_nontemporal_store(s, y + r);
  }
}

// Rows too long for the LDS stage (the matrix's lds_cap is 0): k_spmv_direct's shape, one lane per row, the packed
// words read from global memory, the same order.
__global__ __launch_bounds__(kT) void k_spmv_p32_direct(int32_t nrows, const int32_t* __restrict__ rowptr,
                                                        const uint2* __restrict__ pk, const double* __restrict__ x,
                                                        double* __restrict__ y, const double* __restrict__ sdev,
                                                        const int* __restrict__ stop) {
  if (stopped(stop)) return;
  const int32_t r = blockIdx.x * kT + threadIdx.x;
  if (r >= nrows) return;
  const double sc = *sdev;
  double s = 0.0;
  for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
    const uint2 e = pk[k];
    const double xv = x[(int32_t)e.x] * sc;
    s = s + (double)__uint_as_float(e.y) * xv;
  }
  y[r] = s;
}

}  // namespace
}  // namespace msk

using namespace msk;

extern "C" int msk_csr32_pack(int64_t nnz, const int32_t* col, const double* val, void* pk, unsigned int* over,
                              hipStream_t s) {
  const int64_t g = (nnz + 2 + kT - 1) / kT;
  k_csr32_pack<<<dim3((unsigned)g), dim3(kT), 0, s>>>(nnz, col, val, static_cast<uint2*>(pk), over);
  return (int)hipGetLastError();
}

extern "C" int msk_spmv_p32(int32_t nrows, const int32_t* rowptr, const void* pk, const double* x, double* y,
                            int32_t lds_cap, const double* sdev, const int* stop, int64_t plane, hipStream_t s) {
  if (nrows <= 0) return 0;
  const unsigned g = (unsigned)((nrows + kT - 1) / kT);
  const uint2* p = static_cast<const uint2*>(pk);
  if (lds_cap > 0) {
    int32_t m3[3];
    msk_xcd_map3(nrows, plane, m3);
    const XcdMap xm = {m3[0], m3[1], m3[2]};
    const size_t ldsb = (size_t)((lds_cap + 255) & ~255) * 8;  // slack for the last instruction's tail lanes
    k_spmv_p32<<<dim3(g), dim3(kT), ldsb, s>>>(nrows, rowptr, p, x, y, sdev, stop, xm);
  } else {
    k_spmv_p32_direct<<<dim3(g), dim3(kT), 0, s>>>(nrows, rowptr, p, x, y, sdev, stop);
  }
  return (int)hipGetLastError();
}

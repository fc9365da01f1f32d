// msplit_kdev.hpp -- what more than one of the kernel units of the GMRES inner-solve path (msplit_k_*.hip,
// msplit_kernels.hip) needs: the DBR constants, the small device helpers, the MDot chunk bodies and MAXPY's
// group sum (the dot and MAXPY kernels and the kernels that fuse a MatMult with them) and, for the launchers,
// the tuning flags, the dispatch helper that turns a run-time value into a template argument (pick, pick_range), the
// reader of the environment knobs (env_int) and the MDot stage-1 launch (with the kernel template k_dot_stage1,
// which three units instantiate).  Private to those units: not installed and not included anywhere else.  A helper
// that one unit uses lives in that unit.  tools/launch_table.cpp prints what every launcher of these units picks,
// without a GPU.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "msplit_kernels.h"

namespace msk {
namespace {  // internal linkage: each unit instantiates what it launches, and kernels stay private to their unit

constexpr int kT = 256;                  // threads per workgroup (4 wave64)
constexpr int kIters = 8;                // double2 slices per thread per DBR chunk
constexpr int kChunk = kT * 2 * kIters;  // 4096 elements per DBR chunk

static_assert(kChunk == MSK_DBR_CHUNK, "DBR chunk must match the oracle");

__device__ __forceinline__ bool stopped(const int* stop) { return stop && *stop; }

typedef double dx2 __attribute__((ext_vector_type(2)));
typedef int ix4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double2 ld_nt(const double2* p) {
  const dx2 v = __builtin_nontemporal_load(reinterpret_cast<const dx2*>(p));
  return make_double2(v.x, v.y);
}
__device__ __forceinline__ int4 ld_nt(const int4* p) {
  const ix4 v = __builtin_nontemporal_load(reinterpret_cast<const ix4*>(p));
  return make_int4(v.x, v.y, v.z, v.w);
}

// ---------------------------------------------- the CSR MatMults' row-block schedule and LDS-DMA staging
// (msplit_kernels.hip: k_spmv_lds8 and the box kernels; msplit_csr32.hip: k_spmv_p32).  The XCD-aware order is
// described with the SpMV kernels in msplit_kernels.hip; only the schedule changes, every row's sum is the same.
struct XcdMap {
  int32_t bp;  // row blocks per plane (0: identity order)
  int32_t gb;  // row blocks per group, (bp / gb) % 8 == 0
  int32_t np;  // planes
};

__device__ __forceinline__ int32_t row_block(XcdMap m) {
  const int32_t i = blockIdx.x;
  if (m.bp == 0) return i;
  if (m.bp < 0) return (i & 7) * m.np + (i >> 3);  // z-chunks: XCD x sweeps rows [x N/8, (x+1) N/8) in order
  const int32_t xcd = i & 7, j = i >> 3;
  const int32_t span = m.np * m.gb;  // blocks of one group over all planes
  const int32_t q = j / span, rem = j - q * span;
  const int32_t k = rem / m.gb, t = rem - k * m.gb;
  return k * m.bp + (xcd + 8 * q) * m.gb + t;
}

// aux (cache policy) 2 = nt on gfx950 (global_load_lds_dwordx4 ... nt)
template <bool NT>
__device__ __forceinline__ void glds16(const void* g, void* lds) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)lds, 16, 0, NT ? 2 : 0);
}

__device__ __forceinline__ const double* vec_at(const Vecs& V, int j) {
  return V.base ? V.base + (int64_t)j * V.stride : V.p[j];
}
// deferred VecNormalize: element i of vector j is fl(V_j[i] * scale[j]); x * 1.0
// is exact for every double, so unscaled sets multiply by 1.0 (wave-uniform load)
__device__ __forceinline__ double vec_scale(const Vecs& V, int j) { return V.scale ? V.scale[j] : 1.0; }

// ---------------------------------------------- W = A (sc x) in the CGS kernels
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

// Stage the DV dictionary in LDS (the caller synchronises before use).
__device__ __forceinline__ void ell_dict_stage(const EllOp& op, int32_t* sdel, double* sval) {
  const int t = threadIdx.x;
  if (t < op.ndict) {
    sdel[t] = op.ddelta[t];
    sval[t] = op.dval[t];
  } else {
    sdel[t] = 0;  // code 255 (no entry) and unused codes: delta 0, never added
    sval[t] = 0.0;
  }
}

// The lane's W values at its DBR positions base + j*512 + {0,1}, j in [J0, J0+JN):
// rows e, e+1 read their 2 x 8 codes with one 16-byte load, then every gather
// of the pair is issued before the first product (padding entries gather x[0]
// and are masked out).  Each row sums val * (x * sc) over its entries in CSR
// order from 0.0 -- k_spmv_ell's SCALED sum, term for term.  Rows >= n: 0.
template <int J0, int JN>
__device__ __forceinline__ void ell_rows(const EllOp& op, const int32_t* sdel, const double* sval, double sc,
                                         int64_t base, int64_t n, double (&wr)[2 * kIters]) {
#pragma unroll
  for (int j = J0; j < J0 + JN; ++j) {
    const int64_t e = base + j * (2 * kT);
    u32x4v cw = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (e + 1 < n) {
      cw = __builtin_nontemporal_load(reinterpret_cast<const u32x4v*>(op.code8 + e * 8));
    } else if (e < n) {
      cw.x = reinterpret_cast<const uint32_t*>(op.code8 + e * 8)[0];
      cw.y = reinterpret_cast<const uint32_t*>(op.code8 + e * 8)[1];
    }
    int32_t ix[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const uint32_t w4 = q < 4 ? cw.x : q < 8 ? cw.y : q < 12 ? cw.z : cw.w;
      const int c = (w4 >> (8 * (q & 3))) & 255;
      ix[q] = c != 255 ? (int32_t)(e + (q >> 3)) + sdel[c] : 0;
    }
    double xv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) xv[q] = op.x[ix[q]];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double acc = 0.0;
#pragma unroll
      for (int q = 8 * h; q < 8 * h + 8; ++q) {
        const uint32_t w4 = q < 4 ? cw.x : q < 8 ? cw.y : q < 12 ? cw.z : cw.w;
        const int c = (w4 >> (8 * (q & 3))) & 255;
        const double sn = acc + sval[c] * (xv[q] * sc);
        acc = c != 255 ? sn : acc;
      }
      wr[2 * j + h] = acc;
    }
  }
}

// ---------------------------------------------- box assembly (msplit_kernels.hip, msplit_k_diffusion.hip)
// Row pointers of a box stencil with Dirichlet boundaries in closed form (entries
// before row l = deg*l minus the missing neighbours of rows < l).
__device__ __forceinline__ int64_t box_rowptr(int dim, int64_t l, int64_t nx, int64_t ny, int64_t nz) {
  const int64_t cx0 = (l + nx - 1) / nx, cxN = l / nx;  // rows < l with i == 0 / i == nx-1
  const int64_t P = nx * ny;
  int64_t missing = cx0 + cxN;
  if (dim == 3) {
    const int64_t q = l / P, rem = l % P;
    const int64_t cy0 = q * nx + min(rem, nx);
    const int64_t cyN = q * nx + max((int64_t)0, rem - (ny - 1) * nx);
    const int64_t cz0 = min(l, P);
    const int64_t czN = max((int64_t)0, l - (nz - 1) * P);
    missing += cy0 + cyN + cz0 + czN;
    return 7 * l - missing;
  }
  const int64_t cy0 = min(l, nx);
  const int64_t cyN = max((int64_t)0, l - (ny - 1) * nx);
  missing += cy0 + cyN;
  return 5 * l - missing;
}

__device__ __forceinline__ double wave_butterfly(double v) {
  // v[l] <- v[l] + v[l ^ off], off = 32..1: every lane ends with the same sum.
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// ---------------------------------------------------------------- DBR dots
// Stage 1: workgroup c reduces chunk c of every vector: lane t accumulates its
// elements base + j*512 + 2t, +1 (j = 0..7) in order, wave butterfly, then
// (w0 + w1) + (w2 + w3).  partial[v * nchunks + c].  w stays in registers and
// each vector streams 32 KiB contiguous per workgroup.
// VAR: bit 0 = non-temporal loads of the basis vectors (the default: each
// vector streams through once per kernel and is far larger than the 256 MiB
// MALL, so caching it only evicts lines others still need; +8-16 % per kernel,
// +7.7 % per GMRES step on 256^3, same-box A/B); bit 2 = non-temporal store
// of w in MAXPY.  Results are identical.
// G vectors of a full chunk at once: all G*8 loads are issued before the first
// product (4 x 32 KiB in flight per workgroup instead of one vector's 32 KiB),
// then G independent accumulations and butterflies.  Per vector the sum is the
// same sequence as one at a time.
template <int G, int VAR>
__device__ __forceinline__ void dot_group_full(const double (&wr)[2 * kIters], const Vecs& V, int64_t base, int rev,
                                               int nv, int g, double (*red)[4], int lane, int wv) {
  double2 q[G][kIters];
  double sv[G];
  int vv[G];
#pragma unroll
  for (int u = 0; u < G; ++u) {
    // load order only (each dot is independent): newest vector first when rev
    vv[u] = rev ? nv - 1 - (g + u) : g + u;
    const double* __restrict__ y = vec_at(V, vv[u]);
    sv[u] = vec_scale(V, vv[u]);
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const double2* pq = reinterpret_cast<const double2*>(y + base + j * (2 * kT));
      q[u][j] = (VAR & 1) ? ld_nt(pq) : *pq;
    }
  }
  double acc[G];
#pragma unroll
  for (int u = 0; u < G; ++u) {
    acc[u] = 0.0;
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      acc[u] = acc[u] + wr[2 * j] * (q[u][j].x * sv[u]);
      acc[u] = acc[u] + wr[2 * j + 1] * (q[u][j].y * sv[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < G; ++u) {
    acc[u] = wave_butterfly(acc[u]);
    if (lane == 0) red[vv[u]][wv] = acc[u];
  }
}

// Stage 1: workgroup c reduces chunk c of every vector: lane t accumulates its
// elements base + j*512 + 2t, +1 (j = 0..7) in order, wave butterfly, then
// (w0 + w1) + (w2 + w3).  partial[v * nchunks + c].  w stays in registers and
// each vector streams 32 KiB contiguous per workgroup.
// VAR: bit 0 = non-temporal loads of the basis vectors (the default: each
// vector streams through once per kernel and is far larger than the 256 MiB
// MALL, so caching it only evicts lines others still need; +8-16 % per kernel,
// +7.7 % per GMRES step on 256^3, same-box A/B); bit 2 = non-temporal store
// of w in MAXPY; bit 4 = vectors one at a time in MDot (A/B of the grouped loads).
// Results are identical.
template <int NV, bool SELF, int VAR, bool OPW = false>
__device__ __forceinline__ void dot_chunk(const double* __restrict__ w, const Vecs& V, int64_t n,
                                          double* __restrict__ partial, int64_t nchunks, int rev, int64_t c,
                                          double (&red)[NV][4], const EllOp* op = nullptr,
                                          const int32_t* sdel = nullptr, const double* sval = nullptr) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double wr[2 * kIters];
  if constexpr (OPW) {
    ell_rows<0, kIters>(*op, sdel, sval, *op->sdev, base, n, wr);
  } else if (full) {
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
  if (!SELF && full && (VAR & 16) == 0) {
    constexpr int G = NV >= 4 ? 4 : NV;
    int g = 0;
    if constexpr ((VAR & 32) != 0) {  // two groups per iteration (MSK_TUNE_MDOT_UNROLL2)
#pragma unroll 2
      for (; g + G <= NV; g += G) dot_group_full<G, VAR>(wr, V, base, rev, NV, g, red, lane, wv);
    } else {
#pragma unroll 1
      for (; g + G <= NV; g += G) dot_group_full<G, VAR>(wr, V, base, rev, NV, g, red, lane, wv);
    }
    if constexpr (NV % G == 3) dot_group_full<3, VAR>(wr, V, base, rev, NV, g, red, lane, wv);
    if constexpr (NV % G == 2) dot_group_full<2, VAR>(wr, V, base, rev, NV, g, red, lane, wv);
    if constexpr (NV % G == 1) dot_group_full<1, VAR>(wr, V, base, rev, NV, g, red, lane, wv);
  } else {
#pragma unroll
  for (int vi = 0; vi < NV; ++vi) {
    // load order only (each dot is independent): newest vector first when rev,
    // so the CGS MAXPY that follows finds the oldest ones still in the MALL
    const int v = rev ? NV - 1 - vi : vi;
    double acc = 0.0;
    if (SELF) {
      if (full) {
#pragma unroll
        for (int j = 0; j < 2 * kIters; ++j) acc = acc + wr[j] * wr[j];
      } else {
#pragma unroll
        for (int j = 0; j < kIters; ++j) {
          const int64_t e = base + j * (2 * kT);
          if (e < n) acc = acc + wr[2 * j] * wr[2 * j];
          if (e + 1 < n) acc = acc + wr[2 * j + 1] * wr[2 * j + 1];
        }
      }
    } else {
      const double* __restrict__ y = vec_at(V, v);
      const double sv = vec_scale(V, v);
      if (full) {
        double2 q[kIters];
#pragma unroll
        for (int j = 0; j < kIters; ++j) {
          const double2* pq = reinterpret_cast<const double2*>(y + base + j * (2 * kT));
          q[j] = (VAR & 1) ? ld_nt(pq) : *pq;
        }
#pragma unroll
        for (int j = 0; j < kIters; ++j) {
          acc = acc + wr[2 * j] * (q[j].x * sv);
          acc = acc + wr[2 * j + 1] * (q[j].y * sv);
        }
      } else {
#pragma unroll
        for (int j = 0; j < kIters; ++j) {
          const int64_t e = base + j * (2 * kT);
          if (e < n) acc = acc + wr[2 * j] * (y[e] * sv);
          if (e + 1 < n) acc = acc + wr[2 * j + 1] * (y[e + 1] * sv);
        }
      }
    }
    acc = wave_butterfly(acc);
    if (lane == 0) red[v][wv] = acc;
  }
  }
  __syncthreads();
  if (t < NV) partial[t * nchunks + c] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
}

template <int NV, bool SELF, int VAR>
__global__ __launch_bounds__(kT) void k_dot_stage1(const double* __restrict__ w, Vecs V, int64_t n,
                                                   double* __restrict__ partial, int64_t nchunks,
                                                   const int* __restrict__ stop, int rev) {
  if (stopped(stop)) return;
  __shared__ double red[NV][4];
  dot_chunk<NV, SELF, VAR>(w, V, n, partial, nchunks, rev, blockIdx.x, red);
}

// ------------------------------------------------------------------ MAXPY
// One vector group's sum in PETSc VecMAXPY_Seq's arithmetic (PetscKernelAXPY4/3/2/1), evaluated left to
// right; the grouping is described with chunk_group (msplit_k_maxpy.hip).
template <int G>
__device__ __forceinline__ double group_sum(const double (&a)[G], const double (&p)[G]) {
  if constexpr (G == 1) {
    return a[0] * p[0];
  } else {
    double s = a[0] * p[0] + a[1] * p[1];
    if constexpr (G > 2) s = s + a[2] * p[2];
    if constexpr (G > 3) s = s + a[3] * p[3];
    return s;
  }
}

}  // namespace
}  // namespace msk

// ===================================================================== launchers
// Tuning flags (A/B experiments; MSPLIT_TUNING at context creation), defined in msplit_kernels.hip.
extern __attribute__((visibility("hidden"))) int msk_tuning_flags;
// MAXPY's chunk order, -1 (by size), 0 or 1 (maxpy_rev below), defined in msplit_kernels.hip.
extern __attribute__((visibility("hidden"))) int msk_maxpy_rev_forced;

// The row-block schedule msk_spmv gives an operator of this shape, {bp, gb, np} of XcdMap (msplit_kernels.hip)
__attribute__((visibility("hidden"))) void msk_xcd_map3(int32_t nrows, int64_t plane, int32_t out[3]);

// The A/B variants of MDot stage 1 (msplit_k_dot_a.hip, msplit_k_dot_b.hip), for msk_dot_stage1 (msplit_k_dot.hip).
__attribute__((visibility("hidden"))) int msk_dot1_variants_a(int var, int nv, const double* w, const Vecs& V,
                                                               int64_t n, double* partial, int64_t nchunks,
                                                               const int* stop, hipStream_t s);
__attribute__((visibility("hidden"))) int msk_dot1_variants_b(int var, int nv, const double* w, const Vecs& V,
                                                               int64_t n, double* partial, int64_t nchunks,
                                                               const int* stop, hipStream_t s);

namespace msk {
namespace {

// A run-time value as a template argument: pick<V0, Vs...>(v, f) calls f(std::integral_constant<.., V>{}) for the
// listed V that equals v and returns whether one did; pick_range<LO, HI> lists LO..HI.  f is a generic lambda that
// launches the kernel with decltype(c)::value as the argument.  Only the listed values are instantiated, so a launcher
// lists exactly the kernels that exist, and a value that is not listed launches nothing.
template <auto V0, auto... Vs, class T, class F>
inline bool pick(T v, F&& f) {
  if (v == (T)V0) {
    f(std::integral_constant<decltype(V0), V0>{});
    return true;
  }
  if constexpr (sizeof...(Vs) > 0) return pick<Vs...>(v, f);
  else return false;
}
template <int LO, int HI, class F>
inline bool pick_range(int v, F&& f) {
  if (v == LO) {
    f(std::integral_constant<int, LO>{});
    return true;
  }
  if constexpr (LO < HI) return pick_range<LO + 1, HI>(v, f);
  else return false;
}

// An integer knob of the environment: atoi of its value, dflt where it is not set.
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// basis-vector load policy: non-temporal unless MSK_TUNE_VEC_TEMPORAL (A/B)
inline int vec_var() { return (msk_tuning_flags & MSK_TUNE_VEC_TEMPORAL) ? 0 : 1; }

// MAXPY's chunk order (msk_maxpy_chunk, msk_maxpy_mdot, msk_box_maxpy_march): top chunks first where a vector
// outgrows the 256 MiB MALL (n > 2^25); msk_maxpy_rev_forced (msplit_kernels.hip: MSPLIT_MAXPY_REV, msk_set_maxpy_rev)
// forces either order, -1 leaves it to n.
inline bool maxpy_rev(int64_t n) {
  return msk_maxpy_rev_forced < 0 ? n > ((int64_t)1 << 25) : msk_maxpy_rev_forced != 0;
}

// MDot stage 1 is launched from three units (msplit_k_dot.hip: the default variant; msplit_k_dot_a.hip and
// msplit_k_dot_b.hip: the A/B variants), so the kernel template k_dot_stage1 and this launch are here and each of
// the three instantiates its own variants.  False when nv is not in 1..MSK_MAX_GROUP.
template <int VAR>
bool dot1_launch(int nv, const double* w, const Vecs& V, int64_t n, double* partial, int64_t nchunks, const int* stop,
                 hipStream_t s) {
  return pick_range<1, MSK_MAX_GROUP>(nv, [&](auto k) {
    k_dot_stage1<decltype(k)::value, false, VAR><<<dim3((unsigned)nchunks), dim3(kT), 0, s>>>(
        w, V, n, partial, nchunks, stop, (msk_tuning_flags & MSK_TUNE_MDOT_REV) ? 1 : 0);
  });
}

}  // namespace
}  // namespace msk

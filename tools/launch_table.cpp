// launch_table.cpp -- which kernel every msk_* launcher of the seven kernel units picks, printed without a GPU.
//
// Linked with g++ against csrc/build/{msplit_kernels,msplit_k_dot,msplit_k_dot_op,msplit_k_dot_a,msplit_k_dot_b,
// msplit_k_maxpy,msplit_k_maxpy_mdot}.o and nothing of the HIP runtime: this file defines the handful of runtime
// symbols those objects need.  __hipRegisterFunction learns each host stub's device-side (mangled) name when the
// objects' constructors run; hipLaunchKernel records that name, demangled and cut down to the template and its
// arguments, with the grid, the block and the dynamic LDS size.
// Every launcher is called over a case list that reaches each branch of its dispatch, and one line per case is
// printed: the case key, the return code and the launches ("no launch" when there was none; the block is printed
// unless it is 256 threads, the LDS size unless it is 0).  Pointers are made-up
// addresses, 16-byte aligned or not, that the host code never dereferences; Vecs, Coefs, EllOp and BoxCoef are real.
//
//   launch_table [--brief] [section ...]   the named launchers only (default: all); --brief: fewer cases of the
//                                          large sections; environment knobs come from the caller
//
// Most knobs are read once per process, so a table takes one run per environment setting, with the knob set by the
// caller: profiles/launch_dispatch/README.md has the link line, the settings and the table recorded from the commit
// before the launchers took their present form, to diff a new table against.
#include <cxxabi.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "msplit_kernels.h"

// ------------------------------------------------------------------ the stand-in for the HIP runtime
namespace {
struct Launch {
  std::string name;
  dim3 grid, block;
  size_t lds;
};
std::map<const void*, std::string>& stubs() {  // built on first use: the objects' constructors run before main
  static std::map<const void*, std::string> m;
  return m;
}
// The kernel as the table names it: the demangled name without "void msk::(anonymous namespace)::" and without the
// parameter list and blanks, "k_spmv_lds8<1,3,0>".  No two kernels of the units differ in their parameters alone.
std::string short_name(const char* mangled) {
  int status = 0;
  char* d = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  std::string s = status == 0 && d ? d : mangled;
  free(d);
  const char ns[] = "(anonymous namespace)::";
  const size_t at = s.find(ns);
  if (at != std::string::npos) s.erase(0, at + sizeof ns - 1);
  const size_t paren = s.find('(');
  if (paren != std::string::npos) s.erase(paren);
  s.erase(std::remove(s.begin(), s.end(), ' '), s.end());
  return s;
}
std::vector<Launch> g_launches;
struct {
  dim3 grid, block;
  size_t lds;
  hipStream_t s;
} g_cfg;
}  // namespace

extern "C" {
void** __hipRegisterFatBinary(const void*) {
  static void* handle;
  return &handle;
}
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* device_name, unsigned, void*, void*, void*,
                           void*, int*) {
  stubs()[host] = short_name(device_name);
}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t s) {
  g_cfg = {grid, block, lds, s};
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* s) {
  *grid = g_cfg.grid;
  *block = g_cfg.block;
  *lds = g_cfg.lds;
  *s = g_cfg.s;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t lds, hipStream_t) {
  auto it = stubs().find(f);
  g_launches.push_back({it == stubs().end() ? "?unregistered" : it->second, grid, block, lds});
  return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
}

// hidden in the library, reachable here because the objects are linked in
void msk_xcd_map3(int32_t nrows, int64_t plane, int32_t out[3]);

// ------------------------------------------------------------------ cases
namespace {
int g_cases = 0;
bool g_brief = false;  // --brief: the cases a knob can move, for the runs under an environment setting

void emit(int rc, const char* fmt, ...) {
  char key[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(key, sizeof key, fmt, ap);
  va_end(ap);
  printf("%s | rc=%d |", key, rc);
  if (g_launches.empty()) printf(" no launch");
  for (size_t i = 0; i < g_launches.size(); ++i) {
    const Launch& l = g_launches[i];
    printf("%s %s grid=%u", i ? " ;" : "", l.name.c_str(), l.grid.x);
    if (l.grid.y != 1 || l.grid.z != 1) printf(",%u,%u", l.grid.y, l.grid.z);
    // the usual block of 256 threads and no dynamic LDS are left out
    if (l.block.x != 256 || l.block.y != 1 || l.block.z != 1) printf(" block=%u,%u,%u", l.block.x, l.block.y, l.block.z);
    if (l.lds) printf(" lds=%zu", l.lds);
  }
  printf("\n");
  g_launches.clear();
  ++g_cases;
}
// CASE(call, key format, key values...)
#define CASE(call, ...)   \
  do {                    \
    g_launches.clear();   \
    const int rc_ = (call); \
    emit(rc_, __VA_ARGS__); \
  } while (0)

template <class T = double>
T* al(int i) {  // 16-byte aligned
  return reinterpret_cast<T*>((uintptr_t)0x10000000 + (uintptr_t)0x100000 * i);
}
template <class T = double>
T* mis(int i) {  // 8 bytes past a 16-byte boundary
  return reinterpret_cast<T*>((uintptr_t)0x10000008 + (uintptr_t)0x100000 * i);
}
const char* pn(const void* p) { return !p ? "null" : ((uintptr_t)p & 15) ? "mis" : "al"; }

double* const X = al(1);
double* const B = al(2);
double* const Y = al(3);
double* const VOUT = al(4);
double* const SDEV = al(5);
double* const PART = al(6);
double* const DVAL = al(7);
double* const RV = al(8);
double* const ADEV = al(9);
const uint8_t* const MASK = al<uint8_t>(10);
const uint8_t* const CODE8 = al<uint8_t>(11);
const int32_t* const DDELTA = al<int32_t>(12);
const int32_t* const ROWPTR = al<int32_t>(13);
const int32_t* const COL = al<int32_t>(14);
int* const STOP = al<int>(15);
int* const FAIL = al<int>(16);
const uint8_t* const LEN8 = al<uint8_t>(17);

Vecs table_vecs(const double* last, int nv) {  // an explicit table whose vector nv - 1 is `last`
  Vecs V = {};
  for (int j = 0; j < MSK_MAX_GROUP; ++j) V.p[j] = al(32 + j);
  if (nv >= 1 && nv <= MSK_MAX_GROUP) V.p[nv - 1] = last;
  return V;
}
Vecs strided_vecs(const double* last, int nv, int64_t stride) {
  Vecs V = {};
  V.base = last - (int64_t)(nv - 1) * stride;
  V.stride = stride;
  return V;
}

struct Shape {
  int32_t nx, ny, nz;
};

enum {
  F_MDOT_REV = MSK_TUNE_MDOT_REV, F_TMP = MSK_TUNE_SPMV_TEMPORAL, F_XCD = MSK_TUNE_SPMV_XCD,
  F_STAGE1 = MSK_TUNE_SPMV_STAGE1, F_VT = MSK_TUNE_VEC_TEMPORAL, F_FLAT = MSK_TUNE_BOX_MDOT_FLAT,
  F_TST = MSK_TUNE_MAXPY_TEMPORAL_ST, F_HALVES = MSK_TUNE_MAXPY_HALVES, F_ZCHUNK = MSK_TUNE_SPMV_ZCHUNK,
  F_SINGLE = MSK_TUNE_MDOT_SINGLE, F_G2 = MSK_TUNE_SPMV_MDOT_G2, F_RPL1 = MSK_TUNE_DV_RPL1, F_RPL2 = MSK_TUNE_DV_RPL2,
  F_U1 = MSK_TUNE_MAXPY_UNROLL1, F_MU2 = MSK_TUNE_MDOT_UNROLL2, F_BNOXCD = MSK_TUNE_BOX_MDOT_NOXCD,
  F_TY = MSK_TUNE_ELL_TEMPORAL_Y, F_NTY = MSK_TUNE_SPMV_NTY, F_REG = MSK_TUNE_SPMV_REG_STAGE,
  F_EXON = MSK_TUNE_ELL_XCD_ON, F_EXOFF = MSK_TUNE_ELL_XCD_OFF, F_MOFF = MSK_TUNE_ELL_MARCH_OFF,
  F_MNOXCD = MSK_TUNE_ELL_MARCH_NOXCD
};
// every DV path rejects these two pairs (dv_flags_bad)
const int kDvBad[] = {F_EXON | F_EXOFF, F_MNOXCD | F_MOFF};

void reset() {
  msk_set_tuning(0);
  msk_set_spmv_group(0);
  msk_set_march_z(0);
  msk_set_march_lines(0);
}

// ---- msplit_kernels.hip
void t_blas1() {
  for (int op = -1; op <= 8; ++op) CASE(msk_blas1(op, Y, X, B, 2.0, 1000, nullptr), "op=%d n=1000", op);
  for (int64_t n : {(int64_t)0, (int64_t)-1, (int64_t)1, (int64_t)1 << 22})
    CASE(msk_blas1(MSK_AXPY, Y, X, B, 2.0, n, nullptr), "op=%d n=%lld", MSK_AXPY, (long long)n);
}

void t_stencil_spmv() {
  const BoxCoef cf = {};
  for (int dim : {2, 3})
    for (int mode = 0; mode <= 3; ++mode)
      for (int32_t nx : {600, 601})
        CASE(msk_stencil_spmv(dim, nx, 5, 3, 100, 0, 0, &cf, X, B, Y, mode, SDEV, VOUT, STOP, nullptr),
             "dim=%d mode=%d nx=%d all aligned", dim, mode, nx);
  struct {
    const double *x, *b;
    double *y, *vout;
    int lo;
  } ops[] = {{mis(1), B, Y, VOUT, 0}, {X, mis(2), Y, VOUT, 0}, {X, B, mis(3), VOUT, 0}, {X, B, Y, mis(4), 0},
             {X, nullptr, Y, nullptr, 0}, {X, B, Y, VOUT, 1}};
  for (auto& o : ops)
    for (int mode = 0; mode <= 2; ++mode)
      CASE(msk_stencil_spmv(3, 600, 5, 3, 100, o.lo, 0, &cf, o.x, o.b, o.y, mode, SDEV, o.vout, STOP, nullptr),
           "dim=3 mode=%d nx=600 x=%s b=%s y=%s vout=%s lo=%d", mode, pn(o.x), pn(o.b), pn(o.y), pn(o.vout), o.lo);
  CASE(msk_stencil_spmv(3, 600, 5, 3, 0, 0, 0, &cf, X, B, Y, 0, SDEV, VOUT, STOP, nullptr), "nrows=0");
}

void t_box_stencil() {
  const BoxCoef cf = {};
  for (int64_t nrows : {(int64_t)0, (int64_t)100, (int64_t)1 << 22})
    CASE(msk_box_stencil(3, 8, 8, 8, nrows, 0, 0, &cf, al<int32_t>(13), al<int32_t>(14), Y, nullptr), "nrows=%lld",
         (long long)nrows);
}

void t_spmv_rows() {
  for (int32_t nl : {0, 300})
    for (int resid : {0, 1})
      CASE(msk_spmv_rows(nl, ROWPTR, ROWPTR, COL, DVAL, X, B, Y, resid, nullptr), "nlisted=%d resid=%d", nl, resid);
}

void t_spmm() {
  for (int32_t nrows : {0, 300})
    for (int nc : {0, 4})
      for (int32_t cap : {0, 64}) {
        CASE(msk_spmm(nrows, ROWPTR, COL, DVAL, X, 512, nc, Y, 512, cap, nullptr), "f64 nrows=%d nc=%d lds_cap=%d",
             nrows, nc, cap);
        CASE(msk_spmm_f32(nrows, ROWPTR, COL, DVAL, X, 512, nc, al<float>(3), 512, cap, nullptr),
             "f32 nrows=%d nc=%d lds_cap=%d", nrows, nc, cap);
      }
}

void t_spmm_ell() {
  for (int W : {4, 8, 16, 5})
    for (int32_t nrows : {0, 300})
      for (int nc : {0, 4}) {
        CASE(msk_spmm_ell(nrows, W, CODE8, DDELTA, DVAL, 7, X, 512, nc, Y, 512, nullptr), "f64 W=%d nrows=%d nc=%d", W,
             nrows, nc);
        CASE(msk_spmm_ell_f32(nrows, W, CODE8, DDELTA, DVAL, 7, X, 512, nc, al<float>(3), 512, nullptr),
             "f32 W=%d nrows=%d nc=%d", W, nrows, nc);
      }
}

void t_encode() {
  for (int32_t nrows : {0, 300, 1 << 21}) {
    CASE(msk_ell_encode(nrows, 8, ROWPTR, COL, DVAL, 7, DDELTA, DVAL, al<uint8_t>(11), FAIL, nullptr), "ell nrows=%d",
         nrows);
    CASE(msk_dv_encode(nrows, ROWPTR, COL, DVAL, 7, DDELTA, DVAL, al<uint8_t>(17), al<uint8_t>(11), FAIL, nullptr),
         "dv nrows=%d", nrows);
  }
}

void t_spmv() {
  const int flags[] = {0, F_TMP, F_NTY, F_REG, F_STAGE1, F_TMP | F_NTY, F_REG | F_STAGE1, F_TMP | F_REG,
                       F_TMP | F_STAGE1, F_NTY | F_REG, F_NTY | F_STAGE1, F_XCD, F_ZCHUNK, F_TMP | F_NTY | F_REG | F_STAGE1};
  for (int f : flags) {
    msk_set_tuning(f);
    for (int mode = 0; mode <= 3; ++mode)
      for (int32_t cap : {0, 100, 256}) {
        if (cap != 100 && f != 0) continue;  // the direct kernel and the rounding of the cap: no flag moves them
        CASE(msk_spmv(1000, ROWPTR, COL, DVAL, X, B, Y, cap, mode, SDEV, VOUT, STOP, 0, nullptr),
             "f=0x%x mode=%d lds_cap=%d nrows=1000", f, mode, cap);
      }
  }
  reset();
  CASE(msk_spmv(0, ROWPTR, COL, DVAL, X, B, Y, 100, 0, SDEV, VOUT, STOP, 0, nullptr), "nrows=0");
}

void t_xcd_map() {  // the row-block schedule msk_spmv, msk_spmv_dv and the packed MatMult pass to their kernels
  struct {
    int32_t nrows;
    int64_t plane;
  } sh[] = {{1 << 16, 0}, {1 << 16, 1 << 12}, {1 << 18, 1 << 16}, {(1 << 16) + 256, 1 << 12}, {1 << 16, 1000}, {2049, 0}};
  for (int f : {0, (int)F_XCD, (int)F_ZCHUNK, (int)(F_XCD | F_ZCHUNK)})
    for (int gb : {0, 3})
      for (auto& s : sh) {
        msk_set_tuning(f);
        msk_set_spmv_group(gb);
        int32_t out[3];
        msk_xcd_map3(s.nrows, s.plane, out);
        g_launches.clear();
        emit(0, "f=0x%x group=%d nrows=%d plane=%lld -> bp=%d gb=%d np=%d", f, gb, s.nrows, (long long)s.plane, out[0],
             out[1], out[2]);
      }
  reset();
}

void t_spmv_dv() {
  const int flags[] = {0, F_RPL1, F_RPL2, F_RPL1 | F_RPL2, F_TY, F_TY | F_RPL1, F_TY | F_RPL2, F_EXON, F_EXOFF, F_XCD,
                       kDvBad[0], kDvBad[1]};
  for (int f : flags) {
    msk_set_tuning(f);
    for (int ell_w : {0, 4, 8, 16, 5})
      for (int mode = 0; mode <= 3; ++mode)
        for (int64_t plane : {(int64_t)0, (int64_t)1 << 18}) {
          // the plane size moves only the ELL kernels' block order (an argument, with XCD_ON / _OFF): one mode of it
          if (plane && (mode != 0 || (f != 0 && f != F_EXON && f != F_EXOFF))) continue;
          // these move no template argument: one mode
          if (mode != 0 && (f == F_EXON || f == F_EXOFF || f == F_XCD || f == kDvBad[0] || f == kDvBad[1])) continue;
          if (f != 0 && (mode == 3 || (ell_w == 0 && (f & F_TY)))) continue;  // mode 3 is MULT; CSR order has no y policy
          CASE(msk_spmv_dv(1000, ROWPTR, LEN8, CODE8, DDELTA, DVAL, 7, 100, ell_w, X, B, Y, mode, SDEV, VOUT, STOP,
                           plane, nullptr),
               "f=0x%x ell_w=%d mode=%d plane=%lld", f, ell_w, mode, (long long)plane);
        }
  }
  reset();
  for (int ell_w : {0, 8})
    for (int ndict : {-1, 0, 255, 256, 257})
      CASE(msk_spmv_dv(1000, ROWPTR, LEN8, CODE8, DDELTA, DVAL, ndict, 100, ell_w, X, B, Y, 0, SDEV, VOUT, STOP, 0,
                       nullptr),
           "ell_w=%d ndict=%d", ell_w, ndict);
  for (int ell_w : {0, 8})
    for (int32_t mb : {-1, 0, 5000})
      CASE(msk_spmv_dv(1000, ROWPTR, LEN8, CODE8, DDELTA, DVAL, 7, mb, ell_w, X, B, Y, 0, SDEV, VOUT, STOP, 0, nullptr),
           "ell_w=%d max_block=%d", ell_w, mb);
  CASE(msk_spmv_dv(0, ROWPTR, LEN8, CODE8, DDELTA, DVAL, 7, 100, 8, X, B, Y, 0, SDEV, VOUT, STOP, 0, nullptr), "nrows=0");
}

void t_march_small() {
  for (int32_t nrows : {0, 300})
    for (int d2 : {0, 1}) CASE(msk_march_mask(nrows, d2, CODE8, al<uint8_t>(10), nullptr), "mask nrows=%d d2=%d", nrows, d2);
  CASE(msk_march_check(0, 8, 8, 0, MASK, FAIL, nullptr), "check nrows=0");
  CASE(msk_march_check(300, 0, 8, 0, MASK, FAIL, nullptr), "check nx=0");
  CASE(msk_march_check(300, 8, 0, 0, MASK, FAIL, nullptr), "check ny=0");
  CASE(msk_march_check(300, 8, 8, 1, MASK, FAIL, nullptr), "check nrows=300");
  for (int f : {0, (int)F_MOFF, (int)F_MNOXCD}) {
    msk_set_tuning(f);
    CASE(msk_box_march_pick(8, 8, 8), "pick f=0x%x 8x8x8", f);
    CASE(msk_box_march_pick(8, 0, 8), "pick f=0x%x 8x0x8", f);
  }
  reset();
}

// boxes on either side of every shape predicate of the march launchers: planes of whole DBR chunks or not, nx a
// multiple of 256 or not, odd, above 1024 / 2048, ny below 4, 32 chunks per plane (the XCD order), and sizes past
// INT32_MAX
const Shape kBoxes[] = {{256, 16, 4},   {256, 16, 64},  {100, 10, 4},   {256, 3, 4},     {256, 64, 64}, {512, 256, 8},
                        {2048, 2, 4},   {4096, 1, 4},   {3, 4096, 2},   {1024, 4, 1},    {512, 8, 300}, {256, 256, 256},
                        {2048, 2048, 1024}, {0, 4, 4},  {4, 0, 4},      {4, 4, 0}};

void t_spmv_box_march() {
  for (int lines : {0, 1, 4, 16, 5})
    for (auto& b : kBoxes)
      for (int d2 : {0, 1}) {
        if (g_brief && (lines != 0 || &b - kBoxes >= 6)) continue;
        if (d2 && (lines == 1 || lines == 5)) continue;  // 2D: the overrides 4 and 16 are the ones refused
        if (lines != 0 && (&b - kBoxes >= 6 || (d2 && &b != kBoxes))) continue;  // the overrides: the boxes they move
        msk_set_march_lines(lines);
        CASE(msk_spmv_box_march(b.nx, b.ny, b.nz, d2, MASK, DVAL, X, B, Y, 0, SDEV, VOUT, STOP, nullptr),
             "lines=%d box=%dx%dx%d d2=%d mode=0", lines, b.nx, b.ny, b.nz, d2);
      }
  reset();
  if (g_brief) return;
  const Shape some[] = {{256, 16, 4}, {100, 10, 4}, {256, 64, 64}};
  for (int f : {0, (int)F_TY})
    for (int mode = 0; mode <= 3; ++mode) {
      msk_set_march_lines(4);
      msk_set_tuning(f);
      CASE(msk_spmv_box_march(256, 64, 64, 0, MASK, DVAL, X, B, Y, mode, SDEV, VOUT, STOP, nullptr),
           "lines=4 f=0x%x box=256x64x64 d2=0 mode=%d", f, mode);
    }
  const int flags[] = {0, F_TY, F_MNOXCD, F_MOFF, F_EXON, kDvBad[0], kDvBad[1]};
  for (int lines : {0, 1})
    for (int f : flags)
      for (auto& b : some)
        for (int d2 : {0, 1})
          for (int mode = 0; mode <= 3; ++mode) {
            if (lines == 1 && &b != some) continue;  // lines = 1: the other two take kernels the lines = 0 rows show
            // the flags that move no template argument here: one mode, 3D
            if ((f == F_MNOXCD || f == F_MOFF || f == F_EXON || f == kDvBad[0] || f == kDvBad[1]) && (mode != 0 || d2))
              continue;
            if (d2 && &b != some + 1) continue;  // 2D: one box
            msk_set_march_lines(lines);
            msk_set_tuning(f);
            CASE(msk_spmv_box_march(b.nx, b.ny, b.nz, d2, MASK, DVAL, X, B, Y, mode, SDEV, VOUT, STOP, nullptr),
                 "lines=%d f=0x%x box=%dx%dx%d d2=%d mode=%d", lines, f, b.nx, b.ny, b.nz, d2, mode);
          }
  reset();
  struct {
    const double *x, *b;
    double *y, *vout;
  } ops[] = {{mis(1), B, Y, VOUT}, {X, mis(2), Y, VOUT}, {X, B, mis(3), VOUT}, {X, B, Y, mis(4)}, {X, B, Y, nullptr}};
  for (int lines : {0, 16})
    for (auto& o : ops)
      for (int mode = 0; mode <= 2; ++mode) {
        if (lines == 16 && mode != 0 && &o != ops + 1 && &o != ops + 3) continue;  // b and vout count in one mode each
        msk_set_march_lines(lines);
        CASE(msk_spmv_box_march(256, 16, 4, 0, MASK, DVAL, o.x, o.b, o.y, mode, SDEV, o.vout, STOP, nullptr),
             "lines=%d box=256x16x4 mode=%d x=%s b=%s y=%s vout=%s", lines, mode, pn(o.x), pn(o.b), pn(o.y), pn(o.vout));
      }
  reset();
  for (int z : {1, 2, 64})
    for (int lines : {0, 1, 4})
      for (auto& b : some) {
        msk_set_march_z(z);
        msk_set_march_lines(lines);
        CASE(msk_spmv_box_march(b.nx, b.ny, b.nz, 0, MASK, DVAL, X, B, Y, 0, SDEV, VOUT, STOP, nullptr),
             "march_z=%d lines=%d box=%dx%dx%d", z, lines, b.nx, b.ny, b.nz);
      }
  reset();
}

void t_march_chunk_fits() {
  for (auto& b : kBoxes)
    for (int d2 : {0, 1}) {
      if (g_brief && &b - kBoxes >= 6) continue;
      g_launches.clear();
      emit(msk_march_chunk_fits(b.nx, b.ny, d2), "box=%dx%d d2=%d (rc is the answer)", b.nx, b.ny, d2);
    }
}

void t_box_march_halo() {
  for (auto& b : kBoxes)
    for (int halo = 0; halo <= 3; ++halo) {
      if (halo != 1 && &b != kBoxes) continue;  // the halo bits are a kernel argument: all four on one box
      CASE(msk_box_march_halo(b.nx, b.ny, b.nz, halo, MASK, DVAL, X, B, Y, 0, nullptr), "box=%dx%dx%d halo=%d mode=0",
           b.nx, b.ny, b.nz, halo);
    }
  struct {
    const double *x, *b;
    double* y;
  } ops[] = {{X, B, Y}, {mis(1), B, Y}, {X, mis(2), Y}, {X, B, mis(3)}};
  for (int f : {0, (int)F_TY, (int)F_MNOXCD, kDvBad[0], kDvBad[1]})
    for (auto& o : ops)
      for (int mode = 0; mode <= 2; ++mode)
        for (auto& b : {Shape{256, 16, 4}, Shape{512, 256, 8}}) {
          if (b.nx == 512 && f != 0 && f != F_MNOXCD) continue;  // 32 chunks per plane: the XCD order's flag
          if (f != 0 && f != F_TY && (mode != 0 || &o != ops)) continue;  // these move no template argument
          if (f == F_TY && &o != ops) continue;
          msk_set_tuning(f);
          g_launches.clear();
          if (f == 0 || &o == ops)  // the query the launcher itself asks: alone where it can differ
            emit(msk_box_march_halo_fits(b.nx, b.ny, b.nz, 1, o.x, o.b, o.y, mode),
                 "fits f=0x%x box=%dx%dx%d halo=1 mode=%d x=%s b=%s y=%s (rc is the answer)", f, b.nx, b.ny, b.nz, mode,
                 pn(o.x), pn(o.b), pn(o.y));
          CASE(msk_box_march_halo(b.nx, b.ny, b.nz, 1, MASK, DVAL, o.x, o.b, o.y, mode, nullptr),
               "f=0x%x box=%dx%dx%d halo=1 mode=%d x=%s b=%s y=%s", f, b.nx, b.ny, b.nz, mode, pn(o.x), pn(o.b), pn(o.y));
        }
  reset();
  msk_set_march_z(3);
  CASE(msk_box_march_halo(256, 16, 8, 2, MASK, DVAL, X, B, Y, 1, nullptr), "march_z=3 box=256x16x8 halo=2 mode=1");
  reset();
}

void t_box_march_chunk_rv() {
  for (auto& b : kBoxes) {
    const int64_t n = (int64_t)b.nx * b.ny * b.nz;
    for (int64_t rvs : {n, (int64_t)-1})
      for (int mode = 0; mode <= 3; ++mode) {
        if (mode != 0 && &b != kBoxes && &b != kBoxes + 5) continue;  // every mode on two boxes the kernel takes
        CASE(msk_box_march_chunk_rv(b.nx, b.ny, b.nz, MASK, RV, rvs, X, B, Y, mode, SDEV, VOUT, STOP, nullptr),
             "box=%dx%dx%d rvs=%s mode=%d", b.nx, b.ny, b.nz, rvs < 0 ? "-1" : "n", mode);
      }
  }
  const int64_t n = 256 * 16 * 4;
  for (int64_t rvs : {(int64_t)0, n + 1, n + 2, n - 2, (int64_t)-7})
    CASE(msk_box_march_chunk_rv(256, 16, 4, MASK, RV, rvs, X, B, Y, 0, SDEV, VOUT, STOP, nullptr),
         "box=256x16x4 rvs=%lld (n=%lld)", (long long)rvs, (long long)n);
  struct {
    const double *rv, *x, *b;
    double *y, *vout;
  } ops[] = {{nullptr, X, B, Y, VOUT}, {mis(8), X, B, Y, VOUT}, {RV, mis(1), B, Y, VOUT}, {RV, X, mis(2), Y, VOUT},
             {RV, X, B, mis(3), VOUT}, {RV, X, B, Y, mis(4)},   {RV, X, B, Y, nullptr}};
  for (auto& o : ops)
    for (int mode = 0; mode <= 2; ++mode)
      CASE(msk_box_march_chunk_rv(256, 16, 4, MASK, o.rv, n, o.x, o.b, o.y, mode, SDEV, o.vout, STOP, nullptr),
           "box=256x16x4 rvs=n mode=%d rv=%s x=%s b=%s y=%s vout=%s", mode, pn(o.rv), pn(o.x), pn(o.b), pn(o.y),
           pn(o.vout));
  for (int f : {(int)F_TY, (int)F_MNOXCD, kDvBad[0], kDvBad[1]})
    for (int64_t rvs : {(int64_t)512 * 256 * 8, (int64_t)-1})
      for (int mode = 0; mode <= 2; ++mode) {
        msk_set_tuning(f);
        CASE(msk_box_march_chunk_rv(512, 256, 8, MASK, RV, rvs, X, B, Y, mode, SDEV, VOUT, STOP, nullptr),
             "f=0x%x box=512x256x8 rvs=%s mode=%d", f, rvs < 0 ? "-1" : "n", mode);
      }
  reset();
}

void t_spmv_mdot() {
  for (int f : {0, (int)F_VT, (int)F_G2, (int)(F_VT | F_G2)})
    for (int nv : {0, 1, 7, 32, 33}) {
      msk_set_tuning(f);
      const Vecs V = table_vecs(al(31), nv);
      CASE(msk_spmv_mdot(5000, ROWPTR, COL, DVAL, X, SDEV, Y, 64, &V, nv, PART, 2, STOP, nullptr), "f=0x%x nv=%d", f, nv);
    }
  reset();
  const Vecs V = table_vecs(al(31), 4);
  CASE(msk_spmv_mdot(0, ROWPTR, COL, DVAL, X, SDEV, Y, 64, &V, 4, PART, 2, STOP, nullptr), "nrows=0");
  CASE(msk_spmv_mdot(5000, ROWPTR, COL, DVAL, X, SDEV, Y, 64, &V, 4, PART, 0, STOP, nullptr), "nchunks=0");
  CASE(msk_spmv_mdot(5000, ROWPTR, COL, DVAL, X, SDEV, Y, 0, &V, 4, PART, 2, STOP, nullptr), "lds_cap=0");
}

struct Box2 {
  int32_t nx;
  int64_t P, n;
  int d2;
};
// the (nx, P, n, d2) operands of the fused MatMult+MDot and the W-free MAXPY: marched (planes of whole chunks, n a
// multiple of P, nx even) and not, 32 chunks per plane, nx around 512 / 1024 / 2048, n past 2^25
const Box2 kBox2[] = {{256, 4096, 4096 * 5, 0},      {100, 1000, 4000, 0},            {256, 4096, 4096 * 4, 1},
                      {512, 131072, 131072 * 8, 0},  {514, 514 * 2048, 514 * 2048 * 2, 0}, {256, 65536, (int64_t)65536 * 513, 0},
                      {1024, 4096, 4096 * 6, 0},     {2048, 4096, 4096 * 6, 0},       {256, 4096, 4096 * 4, 0},
                      {256, 4096, 4096 * 4 + 1, 0},  {100, 100, 10000, 1},
                      {3, 3 * 4096, 3 * 4096 * 2, 0}, {1, 4096, 8192, 0},             {2050, 2050 * 2048, 2050 * 2048, 0},
                      {256, 100, 4096, 0},           {256, 4096, 0, 0}};
const int kBrief2 = 6;  // --brief: the first six

void t_box_spmv_mdot() {
  const int flags[] = {0, F_VT | F_TY, F_VT, F_TY, F_FLAT, F_BNOXCD, kDvBad[0], kDvBad[1]};
  for (int f : flags)
    for (auto& b : kBox2)
      for (int self : {0, 1}) {
        if (g_brief && (f != 0 || &b - kBox2 >= kBrief2)) continue;
        // without flags every box, basis ending with x or not; the policies over the first three; the rest over four
        if (f != 0 && (!self || &b - kBox2 >= ((f & ~(F_VT | F_TY)) ? 4 : 3))) continue;
        if (g_brief && (&b == kBox2 + 2 || &b - kBox2 >= 4)) continue;
        msk_set_tuning(f);
        const int nv = 5;
        const Vecs V = table_vecs(self ? X : al(31), nv);
        const int64_t nch = (b.n + MSK_DBR_CHUNK - 1) / MSK_DBR_CHUNK;
        int so = -1;
        g_launches.clear();
        const int rc = msk_box_spmv_mdot(b.nx, b.P, b.n, b.d2, MASK, DVAL, X, SDEV, Y, &V, nv, PART, nch, STOP, &so, nullptr);
        emit(rc, "f=0x%x nx=%d P=%lld n=%lld d2=%d last%sx self_out=%d", f, b.nx, (long long)b.P, (long long)b.n, b.d2,
             self ? "==" : "!=", so);
      }
  reset();
  if (g_brief) return;
  for (int nv : {0, 1, 32, 33}) {
    const Vecs V = table_vecs(X, nv);
    CASE(msk_box_spmv_mdot(256, 4096, 16384, 0, MASK, DVAL, X, SDEV, Y, &V, nv, PART, 4, STOP, nullptr, nullptr),
         "nv=%d table", nv);
    const Vecs S = strided_vecs(X, nv, 1 << 20);
    int so = -1;
    g_launches.clear();
    const int rc = msk_box_spmv_mdot(256, 4096, 16384, 0, MASK, DVAL, X, SDEV, nullptr, &S, nv, PART, 4, nullptr, &so, nullptr);
    emit(rc, "nv=%d strided y=null stop=null self_out=%d", nv, so);
  }
  const Vecs V = table_vecs(X, 5);
  CASE(msk_box_spmv_mdot(256, 4096, 16384, 0, MASK, DVAL, X, SDEV, Y, &V, 5, PART, 0, STOP, nullptr, nullptr), "nchunks=0");
  msk_set_march_z(3);  // not read by this launcher
  CASE(msk_box_spmv_mdot(256, 4096, 16384, 0, MASK, DVAL, X, SDEV, Y, &V, 5, PART, 4, STOP, nullptr, nullptr), "march_z=3");
  reset();
}

void t_box_spmv_mdot_rv() {
  const int flags[] = {0, F_VT, F_TY, F_VT | F_TY, F_FLAT, F_BNOXCD, kDvBad[0]};
  for (int f : flags)
    for (auto& b : kBox2)
      for (int64_t rvs : {b.n, (int64_t)-1}) {
        // without flags every box; with flags a marched box, the 32-chunk one and nx = 514
        if (f != 0 && &b != kBox2 && &b != kBox2 + 3 && &b != kBox2 + 4) continue;
        // --brief: those three without flags; the load / store policies on the first, where the prefetch depth is a
        // template argument (the rows' own values, rvs > 0), and both together on its symmetric form too
        if (g_brief && &b != kBox2 && &b != kBox2 + 3 && &b != kBox2 + 4) continue;
        if (g_brief && f != 0 && ((f & ~(F_VT | F_TY)) || &b != kBox2 || (rvs < 0 && f != (F_VT | F_TY)))) continue;
        msk_set_tuning(f);
        const int nv = 5;
        const Vecs V = table_vecs(X, nv);
        const int64_t nch = (b.n + MSK_DBR_CHUNK - 1) / MSK_DBR_CHUNK;
        int so = -1;
        g_launches.clear();
        const int rc = msk_box_spmv_mdot_rv(b.nx, b.P, b.n, b.d2, MASK, nullptr, RV, rvs, X, SDEV, Y, &V, nv, PART, nch,
                                            STOP, &so, nullptr);
        emit(rc, "f=0x%x nx=%d P=%lld n=%lld d2=%d rvs=%s self_out=%d", f, b.nx, (long long)b.P, (long long)b.n, b.d2,
             rvs < 0 ? "-1" : "n", so);
      }
  reset();
  if (g_brief) return;
  const Vecs V = table_vecs(al(31), 5);
  for (int64_t rvs : {(int64_t)16384, (int64_t)-1})
    CASE(msk_box_spmv_mdot_rv(256, 4096, 16384, 0, MASK, nullptr, RV, rvs, X, SDEV, nullptr, &V, 5, PART, 4, STOP, nullptr,
                              nullptr),
         "rvs=%s y=null", rvs < 0 ? "-1" : "n");
  for (int nv : {0, 1, 32, 33})
    for (int64_t rvs : {(int64_t)16384, (int64_t)-1}) {
      const Vecs T = table_vecs(X, nv);
      CASE(msk_box_spmv_mdot_rv(256, 4096, 16384, 0, MASK, nullptr, RV, rvs, X, SDEV, Y, &T, nv, PART, 4, STOP, nullptr,
                                nullptr),
           "nv=%d rvs=%s", nv, rvs < 0 ? "-1" : "n");
    }
}

void t_box_wfree() {
  for (int on : {-1, 0, 1, 5}) {
    if (on >= 0) msk_set_gm_wfree(on);
    g_launches.clear();
    emit(msk_get_gm_wfree(), "get_gm_wfree after set(%d) (-1: not set; rc is the answer)", on);
    for (int f : {0, kDvBad[0], kDvBad[1]})
      for (auto& b : kBox2) {
        if (g_brief && (f != 0 || on == 5 || &b - kBox2 >= kBrief2)) continue;
        if ((f != 0 || on >= 0) && &b - kBox2 >= 2) continue;  // every box once, then a marched and an unmarched one
        msk_set_tuning(f);
        g_launches.clear();
        emit(msk_box_wfree_fits(b.nx, b.P, b.n, b.d2), "set(%d) f=0x%x nx=%d P=%lld n=%lld d2=%d (rc is the answer)", on, f,
             b.nx, (long long)b.P, (long long)b.n, b.d2);
      }
  }
  reset();
}

void t_box_maxpy_march() {
  g_launches.clear();
  emit(msk_get_maxpy_prefetch(), "get_maxpy_prefetch at start (rc is the answer)");
  const int flags[] = {0, F_VT, F_TST, F_VT | F_TST, F_FLAT, F_BNOXCD, F_TY, kDvBad[0], kDvBad[1]};
  for (int pf : {-1, 0, 1, 2, 3, 4}) {  // -1: the value the environment gave
    if (g_brief && pf != -1 && pf != 2) continue;
    if (pf >= 0) msk_set_maxpy_prefetch(pf);
    g_launches.clear();
    emit(msk_get_maxpy_prefetch(), "get_maxpy_prefetch after set(%d) (rc is the answer)", pf);
    for (int f : flags)
      for (auto& b : kBox2)
        for (int nv : {5, 16}) {
          // With the prefetch mode as the environment left it: every box without flags, the load / store policies
          // and (one nv) the other flags over the first six.  Under each mode set by hand: the first six without
          // flags and the policies on the first.  --brief: what a knob can move.
          const int bi = (int)(&b - kBox2);
          const bool policy = (f & ~(F_VT | F_TST)) == 0;
          bool take;
          if (g_brief)  // the knobs move the marched form only: a small and a large marched box
            take = (bi == 0 || bi == 5) &&
                   (pf == -1 ? f == 0 || f == F_VT || (f == F_TST && bi == 0 && nv == 5) : pf == 2 && f == 0 && nv == 5 && bi == 0);
          else if (pf == -1) take = f == 0 ? nv == 5 || bi == 0 : (policy ? bi < 3 && (nv == 5 || bi == 0) : bi == 0 && nv == 5);
          else take = policy && bi == 0;
          if (!take) continue;
          msk_set_tuning(f);
          const Vecs V = table_vecs(X, nv);
          CASE(msk_box_maxpy_march(b.nx, b.P, b.n, b.d2, MASK, DVAL, X, SDEV, Y, &V, nv, ADEV, PART, STOP, nullptr),
               "prefetch=%d f=0x%x nx=%d P=%lld n=%lld d2=%d nv=%d", pf, f, b.nx, (long long)b.P, (long long)b.n, b.d2, nv);
        }
    msk_set_tuning(0);
    if (g_brief || pf != -1) continue;
    for (int nv : {0, 1, 15, 16, 32, 33, 40}) {
      const Vecs T = table_vecs(X, nv);
      CASE(msk_box_maxpy_march(256, 4096, 16384, 0, MASK, DVAL, X, SDEV, Y, &T, nv, ADEV, PART, STOP, nullptr),
           "prefetch=%d nv=%d table last==x", pf, nv);
      const Vecs S = strided_vecs(X, nv, 1 << 20);
      CASE(msk_box_maxpy_march(256, 4096, 16384, 0, MASK, DVAL, X, SDEV, Y, &S, nv, ADEV, PART, nullptr, nullptr),
           "prefetch=%d nv=%d strided last==x stop=null", pf, nv);
    }
  }
  const Vecs T = table_vecs(al(31), 5);
  CASE(msk_box_maxpy_march(256, 4096, 16384, 0, MASK, DVAL, X, SDEV, Y, &T, 5, ADEV, PART, STOP, nullptr), "table last!=x");
  const Vecs S = strided_vecs(al(31), 5, 1 << 20);
  CASE(msk_box_maxpy_march(256, 4096, 16384, 0, MASK, DVAL, X, SDEV, Y, &S, 5, ADEV, PART, STOP, nullptr), "strided last!=x");
  reset();
}

// ---- the dot and MAXPY units
void t_dot_stage1() {
  const int flags[] = {0, F_VT, F_SINGLE, F_VT | F_SINGLE, F_MU2, F_VT | F_MU2, F_SINGLE | F_MU2,
                       F_VT | F_SINGLE | F_MU2, F_MDOT_REV};
  for (int f : flags) {
    msk_set_tuning(f);
    for (int nv = 0; nv <= MSK_MAX_GROUP + 1; ++nv) {
      // every nv for the six variants that exist; one for the sets with no kernel and for the flag that is an argument
      if (((f & F_SINGLE) && (f & F_MU2)) || f == F_MDOT_REV) {
        if (nv != 5) continue;
      }
      const Vecs V = table_vecs(al(31), nv);
      CASE(msk_dot_stage1(X, &V, nv, 40000, PART, 10, 0, STOP, nullptr), "f=0x%x nv=%d", f, nv);
    }
    const Vecs V = table_vecs(al(31), 1);
    for (int nv : {0, 1, 40}) CASE(msk_dot_stage1(X, &V, nv, 40000, PART, 10, 1, STOP, nullptr), "f=0x%x self nv=%d", f, nv);
  }
  reset();
  const Vecs V = table_vecs(al(31), 3);
  CASE(msk_dot_stage1(X, &V, 3, 40000, PART, 0, 0, STOP, nullptr), "nchunks=0");
  CASE(msk_dot_stage1(X, &V, 3, 40000, PART, 10, 0, nullptr, nullptr), "stop=null");
}

void t_dot_stage2() {
  for (int nv : {1, 32})
    for (const int* stop : {(const int*)nullptr, (const int*)STOP})
      CASE(msk_dot_stage2(PART, 10, nv, Y, stop, nullptr), "nv=%d stop=%s", nv, pn(stop));
}

void t_dot_stage1_op() {
  EllOp op = {CODE8, DDELTA, DVAL, 7, X, SDEV};
  for (int f : {0, (int)F_VT, (int)F_SINGLE, (int)F_MU2}) {
    msk_set_tuning(f);
    for (int nv = 0; nv <= MSK_MAX_GROUP + 1; ++nv) {
      if ((f == F_SINGLE || f == F_MU2) && nv != 5) continue;  // flags this launcher does not read
      const Vecs V = table_vecs(al(31), nv);
      CASE(msk_dot_stage1_op(&op, &V, nv, 40000, PART, 10, STOP, nullptr), "f=0x%x nv=%d", f, nv);
    }
  }
  reset();
  const Vecs V = table_vecs(al(31), 3);
  for (int ndict : {255, 256}) {
    op.ndict = ndict;
    CASE(msk_dot_stage1_op(&op, &V, 3, 40000, PART, 10, STOP, nullptr), "ndict=%d", ndict);
  }
  CASE(msk_dot_stage1_op(&op, &V, 3, 40000, PART, 0, STOP, nullptr), "nchunks=0");
}

void t_maxpy_op() {
  EllOp op = {CODE8, DDELTA, DVAL, 7, X, SDEV};
  const Vecs V = table_vecs(al(31), 5);
  for (int f : {0, (int)F_VT, (int)F_TST, (int)(F_VT | F_TST), (int)F_HALVES, (int)F_U1}) {
    msk_set_tuning(f);
    CASE(msk_maxpy_op(&op, Y, &V, 5, ADEV, 40000, PART, STOP, nullptr), "f=0x%x nv=5 n=40000", f);
  }
  reset();
  CASE(msk_maxpy_op(&op, Y, &V, 0, ADEV, 40000, PART, STOP, nullptr), "nv=0");
  CASE(msk_maxpy_op(&op, Y, &V, 5, ADEV, 0, PART, STOP, nullptr), "n=0");
  for (int ndict : {255, 256}) {
    op.ndict = ndict;
    CASE(msk_maxpy_op(&op, Y, &V, 5, ADEV, 4096, PART, STOP, nullptr), "ndict=%d n=4096", ndict);
  }
}

void t_maxpy_chunk() {
  const Coefs A = {};
  const Vecs V = table_vecs(al(31), 5);
  for (int m = 0; m < 16; ++m) {
    const int f = ((m & 1) ? F_VT : 0) | ((m & 2) ? F_TST : 0) | ((m & 4) ? F_HALVES : 0) | ((m & 8) ? F_U1 : 0);
    if (g_brief && (m & ~2)) continue;
    msk_set_tuning(f);
    for (int64_t n : {(int64_t)40000, ((int64_t)1 << 25), ((int64_t)1 << 25) + 1})
      for (int form = 0; form < 4; ++form) {  // bit 0: the ||w||^2 partials, bit 1: accum
        // past 2^25 only the order changes: one form there, and the boundary itself without flags
        if (n > 40000 && form != 0 && m != 0 && m != 2) continue;  // 0 and 2: the variants with a reversed form
        if (n == ((int64_t)1 << 25) && (m != 0 || form != 0)) continue;
        if (form == 3 && m != 0) continue;  // partials and accum: the partials win
        if (g_brief && form != 0) continue;
        double* partial = (form & 1) ? PART : nullptr;
        CASE(msk_maxpy_chunk(X, Y, &V, 5, nullptr, &A, ADEV, 1, n, form >> 1, partial, STOP, nullptr),
             "f=0x%x n=%lld partial=%s accum=%d", f, (long long)n, pn(partial), form >> 1);
      }
  }
  reset();
  CASE(msk_maxpy_chunk(X, Y, &V, 5, nullptr, &A, ADEV, 1, 0, 0, nullptr, STOP, nullptr), "n=0");
  CASE(msk_maxpy_chunk(X, Y, &V, 0, nullptr, &A, ADEV, 1, 40000, 0, nullptr, STOP, nullptr), "nv=0 nvdev=null");
  CASE(msk_maxpy_chunk(X, Y, &V, 0, STOP, &A, nullptr, 0, 40000, 1, nullptr, nullptr, nullptr), "nv=0 nvdev set accum=1");
}

void t_maxpy_mdot() {
  for (int f : {0, (int)F_TST, (int)F_VT}) {
    msk_set_tuning(f);
    for (int nv = 0; nv <= MSK_MAX_GROUP; ++nv) {
      if (f == F_VT && nv != 5) continue;  // a flag this launcher does not read
      const Vecs V = table_vecs(al(31), nv);
      CASE(msk_maxpy_mdot(X, Y, &V, nv, ADEV, 40000, PART, 10, STOP, nullptr), "f=0x%x nv=%d", f, nv);
    }
  }
  reset();
  const Vecs V = table_vecs(al(31), 3);
  CASE(msk_maxpy_mdot(X, Y, &V, 3, ADEV, 0, PART, 10, STOP, nullptr), "n=0");
  CASE(msk_maxpy_mdot(X, Y, &V, 3, ADEV, 40000, PART, 0, STOP, nullptr), "nchunks=0");
  CASE(msk_maxpy_mdot(X, Y, &V, 3, ADEV, ((int64_t)1 << 25) + 1, PART, 8193, STOP, nullptr), "n=2^25+1 (rev is a kernel argument)");
}

const struct {
  const char* name;
  void (*run)();
} kSections[] = {{"msk_blas1", t_blas1},
                 {"msk_stencil_spmv", t_stencil_spmv},
                 {"msk_box_stencil", t_box_stencil},
                 {"msk_spmv_rows", t_spmv_rows},
                 {"msk_spmm", t_spmm},
                 {"msk_spmm_ell", t_spmm_ell},
                 {"msk_encode", t_encode},
                 {"msk_spmv", t_spmv},
                 {"msk_xcd_map3", t_xcd_map},
                 {"msk_spmv_dv", t_spmv_dv},
                 {"msk_march_small", t_march_small},
                 {"msk_spmv_box_march", t_spmv_box_march},
                 {"msk_march_chunk_fits", t_march_chunk_fits},
                 {"msk_box_march_halo", t_box_march_halo},
                 {"msk_box_march_chunk_rv", t_box_march_chunk_rv},
                 {"msk_spmv_mdot", t_spmv_mdot},
                 {"msk_box_spmv_mdot", t_box_spmv_mdot},
                 {"msk_box_spmv_mdot_rv", t_box_spmv_mdot_rv},
                 {"msk_box_wfree_fits", t_box_wfree},
                 {"msk_box_maxpy_march", t_box_maxpy_march},
                 {"msk_dot_stage1", t_dot_stage1},
                 {"msk_dot_stage2", t_dot_stage2},
                 {"msk_dot_stage1_op", t_dot_stage1_op},
                 {"msk_maxpy_op", t_maxpy_op},
                 {"msk_maxpy_chunk", t_maxpy_chunk},
                 {"msk_maxpy_mdot", t_maxpy_mdot}};
}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--brief")) {
    g_brief = true;
    --argc;
    ++argv;
  }
  for (int i = 1; i < argc; ++i) {
    bool known = false;
    for (auto& s : kSections) known = known || !strcmp(s.name, argv[i]);
    if (!known) {
      fprintf(stderr, "launch_table: no section %s\n", argv[i]);
      return 2;
    }
  }
  for (auto& s : kSections) {
    bool want = argc == 1;
    for (int i = 1; i < argc; ++i) want = want || !strcmp(s.name, argv[i]);
    if (!want) continue;
    printf("## %s\n", s.name);
    reset();
    s.run();
  }
  // the kernels the objects registered, for the coverage count
  for (auto& kv : stubs()) fprintf(stderr, "registered %s\n", kv.second.c_str());
  fprintf(stderr, "launch_table: %d cases, %zu kernels registered\n", g_cases, stubs().size());
  return 0;
}

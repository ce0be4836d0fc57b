// libspx.so -- MI355X (gfx950) tile-execution kernels behind include/spx.h.
//
// This file holds the ahead-of-time kernels (fills, reduction finalize, tile
// merge, region copy, MFMA GEMM dispatch, arg-reduction combine), includes the
// k-means, scan, sort and index families (kmeans_kernels.h, scan_kernels.h,
// sort_kernels.h, index_kernels.h, stencil_kernels.h) and the module/launch
// plumbing for the fused map / map+reduce kernels that spartan_amd/codegen.py
// generates per expression.  Reference call sites replaced are cited per
// entry point in include/spx.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/spx.h"

typedef int64_t i64;
typedef uint64_t u64;

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;

static int set_err(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                         \
  do {                                                                        \
    hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess)                                                     \
      return set_err(SPX_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

#define LAUNCH_CHECK(name)                                                    \
  do {                                                                        \
    hipError_t e_ = hipGetLastError();                                        \
    if (e_ != hipSuccess)                                                     \
      return set_err(SPX_EHIP, "%s launch failed: %s", name,                  \
                     hipGetErrorString(e_));                                  \
  } while (0)

extern "C" int spx_abi_version(void) { return SPX_ABI_VERSION; }
extern "C" const char* spx_last_error(void) { return g_err.c_str(); }
// error text from the host-only translation units (comm.cpp)
extern "C" int spx_comm_set_error(const char* msg) {
  g_err = msg ? msg : "";
  return 0;
}

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

static bool valid_dtype(int d) { return d >= SPX_BOOL && d <= SPX_F64; }

// ----------------------------------------------------- dtype-generic access
// Used by the non-hot-path kernels (merge / copy / finalize) where a uniform
// per-element switch is cheaper than instantiating every dtype pair.
__device__ __forceinline__ double ld_f(const void* p, int dt, i64 i) {
  switch (dt) {
    case SPX_BOOL: return (double)((const uint8_t*)p)[i];
    case SPX_I32: return (double)((const int32_t*)p)[i];
    case SPX_I64: return (double)((const int64_t*)p)[i];
    case SPX_F32: return (double)((const float*)p)[i];
    default: return ((const double*)p)[i];
  }
}
__device__ __forceinline__ i64 ld_i(const void* p, int dt, i64 i) {
  switch (dt) {
    case SPX_BOOL: return (i64)((const uint8_t*)p)[i];
    case SPX_I32: return (i64)((const int32_t*)p)[i];
    case SPX_I64: return ((const int64_t*)p)[i];
    case SPX_F32: return (i64)((const float*)p)[i];
    default: return (i64)((const double*)p)[i];
  }
}
__device__ __forceinline__ bool is_float_dt(int dt) { return dt == SPX_F32 || dt == SPX_F64; }

__device__ __forceinline__ void st_f(void* p, int dt, i64 i, double v) {
  switch (dt) {
    case SPX_BOOL: ((uint8_t*)p)[i] = (v != 0.0); break;
    case SPX_I32: ((int32_t*)p)[i] = (int32_t)(i64)v; break;
    case SPX_I64: ((int64_t*)p)[i] = (i64)v; break;
    case SPX_F32: ((float*)p)[i] = (float)v; break;
    default: ((double*)p)[i] = v; break;
  }
}
__device__ __forceinline__ void st_i(void* p, int dt, i64 i, i64 v) {
  switch (dt) {
    case SPX_BOOL: ((uint8_t*)p)[i] = (v != 0); break;
    case SPX_I32: ((int32_t*)p)[i] = (int32_t)v; break;  // wraps like astype
    case SPX_I64: ((int64_t*)p)[i] = v; break;
    case SPX_F32: ((float*)p)[i] = (float)v; break;
    default: ((double*)p)[i] = (double)v; break;
  }
}

struct Geom {  // up to 8-d row-major geometry passed by value
  int ndim;
  i64 a[8];
  i64 b[8];
  i64 c[8];
  i64 d[8];
};

static int grid_for(i64 n, int per_thread = 1) {
  i64 g = (n + 256LL * per_thread - 1) / (256LL * per_thread);
  if (g < 1) g = 1;
  if (g > 65536) g = 65536;
  return (int)g;
}

// Streamed once-read loads carry the non-temporal hint (global_load ... nt;
// measured +5-9 % on the generated streaming kernels).
template <typename T>
__device__ __forceinline__ T ld_stream(const T* p) {
  return __builtin_nontemporal_load(p);
}

// =================================================================== fills
__device__ __forceinline__ u64 mix64(u64 z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
// counter-based splitmix64 stream: value at global flat index g
__device__ __forceinline__ u64 rng_at(u64 seed, u64 g) {
  return mix64(seed * 0xD1B54A32D192ED03ULL + (g + 1ULL) * 0x9E3779B97F4A7C15ULL);
}

// standard normal at global flat index g: Box-Muller over the two counter
// streams 2g (u1 in (0,1]) and 2g+1 (u2 in [0,1)), computed in fp64
__device__ __forceinline__ double normal_at(u64 seed, i64 g) {
  double u1 = (double)((rng_at(seed, 2ULL * (u64)g) >> 11) + 1ULL) * 1.1102230246251565e-16;
  double u2 = (double)(rng_at(seed, 2ULL * (u64)g + 1ULL) >> 11) * 1.1102230246251565e-16;
  double r = sqrt(-2.0 * log(u1));
  return r * cos(6.283185307179586 * u2);
}

template <typename T>
__device__ __forceinline__ T fill_value(int kind, int dt, double a, double b, u64 seed, i64 g);

template <>
__device__ __forceinline__ float fill_value<float>(int kind, int, double a, double b, u64 seed, i64 g) {
  if (kind == SPX_FILL_CONST) return (float)a;
  if (kind == SPX_FILL_ARANGE) return (float)(a + b * (double)g);
  if (kind == SPX_FILL_NORMAL) return (float)(a + b * normal_at(seed, g));
  float u = (float)(rng_at(seed, (u64)g) >> 40) * 5.9604644775390625e-08f;  // 2^-24
  float lo = (float)a, span = (float)(b - a);
  float t = span * u;  // separate rounding steps (fp-contract off) -- oracle does the same
  return lo + t;
}
template <>
__device__ __forceinline__ double fill_value<double>(int kind, int, double a, double b, u64 seed, i64 g) {
  if (kind == SPX_FILL_CONST) return a;
  if (kind == SPX_FILL_ARANGE) return a + b * (double)g;
  if (kind == SPX_FILL_NORMAL) return a + b * normal_at(seed, g);
  double u = (double)(rng_at(seed, (u64)g) >> 11) * 1.1102230246251565e-16;  // 2^-53
  double t = (b - a) * u;
  return a + t;
}
__device__ __forceinline__ i64 sat_i64(double a) {  // saturating double -> int64
  if (a >= 9.2233720368547758e18) return 0x7fffffffffffffffLL;
  if (a <= -9.2233720368547758e18) return (i64)(-0x7fffffffffffffffLL - 1);
  return (i64)a;
}
template <typename T>
__device__ __forceinline__ T fill_value_int(int kind, double a, double b, u64 seed, i64 g) {
  if (kind == SPX_FILL_CONST) return (T)sat_i64(a);
  if (kind == SPX_FILL_ARANGE) return (T)((i64)a + (i64)b * g);
  if (kind == SPX_FILL_NORMAL) return (T)(i64)floor(a + b * normal_at(seed, g));
  double u = (double)(rng_at(seed, (u64)g) >> 11) * 1.1102230246251565e-16;
  return (T)(i64)floor(a + (b - a) * u);
}

template <typename T>
__global__ __launch_bounds__(256) void k_fill(T* out, i64 n, Geom geo, int contiguous, i64 base,
                                              int kind, int dt, double a, double b, u64 seed) {
  i64 stride = (i64)gridDim.x * 256;
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
    i64 g;
    if (contiguous) {
      g = base + e;
    } else {  // unravel over tile shape (a), shift by ul (b), ravel over array shape (c)
      i64 rem = e, mul = 1;
      g = 0;
      for (int d = geo.ndim - 1; d >= 0; --d) {
        i64 li = rem % geo.a[d];
        rem /= geo.a[d];
        g += (li + geo.b[d]) * mul;
        mul *= geo.c[d];
      }
    }
    T v;
    if constexpr (sizeof(T) == 4 && (T)0.5f != (T)0) v = fill_value<float>(kind, dt, a, b, seed, g);
    else if constexpr (sizeof(T) == 8 && (T)0.5 != (T)0) v = fill_value<double>(kind, dt, a, b, seed, g);
    else v = fill_value_int<T>(kind, a, b, seed, g);
    out[e] = v;
  }
}

extern "C" int spx_fill(int dtype, int kind, void* out, int ndim, const int64_t* tile_shape,
                        const int64_t* ul, const int64_t* array_shape, double a, double b,
                        uint64_t seed, void* stream) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_fill: bad dtype %d", dtype);
  if (ndim < 0 || ndim > 8) return set_err(SPX_EINVAL, "spx_fill: ndim %d > 8", ndim);
  if (kind < SPX_FILL_CONST || kind > SPX_FILL_NORMAL)
    return set_err(SPX_EINVAL, "spx_fill: bad kind %d", kind);
  Geom geo{};
  geo.ndim = ndim;
  i64 n = 1;
  for (int d = 0; d < ndim; ++d) {
    geo.a[d] = tile_shape[d] > 0 ? tile_shape[d] : 1;
    geo.b[d] = ul[d];
    geo.c[d] = array_shape[d] > 0 ? array_shape[d] : 1;
    n *= tile_shape[d];
  }
  if (n == 0) return SPX_OK;
  if (!out) return set_err(SPX_EINVAL, "spx_fill: null output");
  // contiguous in the global flat index iff all dims after the first equal the array's
  int contiguous = 1;
  for (int d = 1; d < ndim; ++d)
    if (geo.a[d] != geo.c[d] || geo.b[d] != 0) contiguous = 0;
  i64 base = 0, mul = 1;
  for (int d = ndim - 1; d >= 0; --d) {
    base += geo.b[d] * mul;
    mul *= geo.c[d];
  }
  int g = grid_for(n, 4);
  switch (dtype) {
    case SPX_F32: k_fill<float><<<g, 256, 0, S(stream)>>>((float*)out, n, geo, contiguous, base, kind, dtype, a, b, seed); break;
    case SPX_F64: k_fill<double><<<g, 256, 0, S(stream)>>>((double*)out, n, geo, contiguous, base, kind, dtype, a, b, seed); break;
    case SPX_I32: k_fill<int32_t><<<g, 256, 0, S(stream)>>>((int32_t*)out, n, geo, contiguous, base, kind, dtype, a, b, seed); break;
    case SPX_I64: k_fill<int64_t><<<g, 256, 0, S(stream)>>>((int64_t*)out, n, geo, contiguous, base, kind, dtype, a, b, seed); break;
    default: k_fill<uint8_t><<<g, 256, 0, S(stream)>>>((uint8_t*)out, n, geo, contiguous, base, kind, dtype, a, b, seed); break;
  }
  LAUNCH_CHECK("spx_fill");
  return SPX_OK;
}

// ======================================================== reduce finalize
__device__ __forceinline__ bool dnan(double x) { return x != x; }

__device__ __forceinline__ double comb_f(int op, double acc, double v) {
  if (op == SPX_OP_SUM) return acc + v;
  if (dnan(acc) || dnan(v)) return dnan(acc) ? acc : v;  // NaN propagates (np.minimum)
  if (op == SPX_OP_MIN) return v < acc ? v : acc;
  return v > acc ? v : acc;
}
__device__ __forceinline__ i64 comb_i(int op, i64 acc, i64 v) {
  if (op == SPX_OP_SUM) return (i64)((u64)acc + (u64)v);
  if (op == SPX_OP_MIN) return v < acc ? v : acc;
  return v > acc ? v : acc;
}
// index value marking an empty (value, index) slot: never wins, always loses
#define ARG_EMPTY 0x7fffffffffffffffLL
// (value, index) "is candidate better than best" for ARGMIN/ARGMAX with
// numpy's NaN rule (first NaN wins) and first-index tie break.
__device__ __forceinline__ bool arg_better(int op, double v, i64 vi, double b, i64 bi) {
  bool vn = dnan(v), bn = dnan(b);
  if (vn || bn) {
    if (vn && !bn) return true;
    if (!vn && bn) return false;
    return vi < bi;
  }
  if (v == b) return vi < bi;
  return op == SPX_OP_ARGMIN ? (v < b) : (v > b);
}
// integer values compare as int64 (a double compare would merge distinct
// values above 2^53 and hand the tie to the lower index)
__device__ __forceinline__ bool arg_better_i(int op, i64 v, i64 vi, i64 b, i64 bi) {
  if (v == b) return vi < bi;
  return op == SPX_OP_ARGMIN ? (v < b) : (v > b);
}
// fold partial p = (v, vi) into the running best (b, bi); ARG_EMPTY slots
// never win
template <typename V>
__device__ __forceinline__ void arg_fold(int op, V v, i64 vi, V& b, i64& bi) {
  bool better;
  if constexpr (std::is_same<V, double>::value) better = arg_better(op, v, vi, b, bi);
  else better = arg_better_i(op, v, vi, b, bi);
  if (vi != ARG_EMPTY && (bi == ARG_EMPTY || better)) { b = v; bi = vi; }
}

// Block ``blk`` of ``nblk`` 256-thread blocks: one thread per output, the P
// partials folded in p order (k_finalize, and the column half of
// k_finalize_pair).
__device__ __forceinline__ void finalize_thin(int op, int acc_dt, int out_dt, const void* pv, const i64* pi, i64 P,
                                              i64 n, void* out, void* out_val, i64 blk, i64 nblk) {
  i64 stride = nblk * 256;
  for (i64 i = blk * 256 + threadIdx.x; i < n; i += stride) {
    if ((op == SPX_OP_ARGMIN || op == SPX_OP_ARGMAX) && is_float_dt(acc_dt)) {
      double b = ld_f(pv, acc_dt, i);
      i64 bi = pi[i];
      for (i64 p = 1; p < P; ++p) arg_fold(op, ld_f(pv, acc_dt, p * n + i), pi[p * n + i], b, bi);
      ((i64*)out)[i] = bi;
      if (out_val) st_f(out_val, acc_dt, i, b);
    } else if (op == SPX_OP_ARGMIN || op == SPX_OP_ARGMAX) {
      i64 b = ld_i(pv, acc_dt, i);
      i64 bi = pi[i];
      for (i64 p = 1; p < P; ++p) arg_fold(op, ld_i(pv, acc_dt, p * n + i), pi[p * n + i], b, bi);
      ((i64*)out)[i] = bi;
      if (out_val) st_i(out_val, acc_dt, i, b);
    } else if (is_float_dt(acc_dt)) {
      double acc = ld_f(pv, acc_dt, i);
      if (acc_dt == SPX_F32) {  // keep fp32 rounding of each step for fp32 accumulators
        float facc = (float)acc;
        for (i64 p = 1; p < P; ++p) {
          float v = ((const float*)pv)[p * n + i];
          facc = (op == SPX_OP_SUM) ? facc + v : (float)comb_f(op, (double)facc, (double)v);
        }
        acc = facc;
      } else {
        for (i64 p = 1; p < P; ++p) acc = comb_f(op, acc, ld_f(pv, acc_dt, p * n + i));
      }
      if (is_float_dt(out_dt)) st_f(out, out_dt, i, acc);
      else st_i(out, out_dt, i, (i64)acc);
    } else {
      i64 acc = ld_i(pv, acc_dt, i);
      for (i64 p = 1; p < P; ++p) acc = comb_i(op, acc, ld_i(pv, acc_dt, p * n + i));
      st_i(out, out_dt, i, acc);
    }
  }
}

__global__ __launch_bounds__(256) void k_finalize(int op, int acc_dt, int out_dt, const void* pv,
                                                  const i64* pi, i64 P, i64 n, void* out,
                                                  void* out_val) {
  finalize_thin(op, acc_dt, out_dt, pv, pi, P, n, out, out_val, blockIdx.x, gridDim.x);
}

// Many partials per output (a tall column reduce splits R over P ~ 2048
// blocks, e.g. cfg5's (1e8, 64) gradient): one block per output, threads
// stride over P in order, then a fixed-shape LDS tree -- deterministic run to
// run.  Float partials are combined in fp64.
// (finalize_wide: block ``blk`` of ``nblk``; k_finalize_wide, and the column
// half of k_finalize_pair)
__device__ __forceinline__ void finalize_wide(int op, int acc_dt, int out_dt, const void* pv, const i64* pi, i64 P,
                                              i64 n, void* out, void* out_val, i64 blk, i64 nblk) {
  __shared__ double sv[256];
  __shared__ i64 si[256];
  __shared__ i64 sw[256];  // integer arg values (compared as int64)
  const int t = threadIdx.x;
  const bool arg = op == SPX_OP_ARGMIN || op == SPX_OP_ARGMAX;
  const bool fl = is_float_dt(acc_dt);
  for (i64 i = blk; i < n; i += nblk) {
    double b = 0.0;
    i64 bw = 0;
    i64 bi = ARG_EMPTY;
    bool have = false;
    for (i64 p = t; p < P; p += 256) {
      if (arg && fl) {
        arg_fold(op, ld_f(pv, acc_dt, p * n + i), pi[p * n + i], b, bi);
      } else if (arg) {
        arg_fold(op, ld_i(pv, acc_dt, p * n + i), pi[p * n + i], bw, bi);
      } else if (fl) {
        double v = ld_f(pv, acc_dt, p * n + i);
        b = have ? comb_f(op, b, v) : v;
      } else {
        i64 v = ld_i(pv, acc_dt, p * n + i);
        bi = have ? comb_i(op, bi, v) : v;
      }
      have = true;
    }
    sv[t] = b;
    si[t] = bi;
    sw[t] = bw;
    __syncthreads();
    // lanes with no partial (P < 256) hold have=false: they are skipped by
    // letting the tree only combine slots < min(P, 256)
    const int m = P < 256 ? (int)P : 256;
    for (int h = 128; h > 0; h >>= 1) {
      if (t < h && t + h < m) {
        if (arg && fl) {
          double vb = sv[t];
          i64 ib = si[t];
          arg_fold(op, sv[t + h], si[t + h], vb, ib);
          sv[t] = vb;
          si[t] = ib;
        } else if (arg) {
          i64 vb = sw[t];
          i64 ib = si[t];
          arg_fold(op, sw[t + h], si[t + h], vb, ib);
          sw[t] = vb;
          si[t] = ib;
        } else if (fl) {
          sv[t] = comb_f(op, sv[t], sv[t + h]);
        } else {
          si[t] = comb_i(op, si[t], si[t + h]);
        }
      }
      __syncthreads();
    }
    if (t == 0) {
      if (arg) {
        ((i64*)out)[i] = si[0];
        if (out_val) {
          if (fl) st_f(out_val, acc_dt, i, sv[0]);
          else st_i(out_val, acc_dt, i, sw[0]);
        }
      } else if (fl) {
        if (is_float_dt(out_dt)) st_f(out, out_dt, i, sv[0]);
        else st_i(out, out_dt, i, (i64)sv[0]);
      } else {
        st_i(out, out_dt, i, si[0]);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_finalize_wide(int op, int acc_dt, int out_dt, const void* pv,
                                                       const i64* pi, i64 P, i64 n, void* out,
                                                       void* out_val) {
  finalize_wide(op, acc_dt, out_dt, pv, pi, P, n, out, out_val, blockIdx.x, gridDim.x);
}

// Whether spx_reduce_finalize folds [P][n] partials with k_finalize_wide, and
// the grid of either kernel.
static bool finalize_is_wide(i64 P, i64 n) { return P >= 32 && n <= 16384; }
static unsigned finalize_grid(i64 P, i64 n) {
  return finalize_is_wide(P, n) ? (unsigned)(n < 4096 ? n : 4096) : (unsigned)grid_for(n);
}

// The two partial sets of a paired column + row sum (codegen.gen_reduce
// pair=True) in one launch.  Blocks [0, gc): the column partials [P][n],
// exactly as spx_reduce_finalize folds them (same kernel body, same grid, so
// bit-identical).  Blocks [gc, gc + gr): the row partials [CT][R], each row
// folded in ct order in an fp64 accumulator and rounded once to the value
// type (fp64 values: folded in fp64).  A block takes PAIR_ROWS consecutive
// rows: all 256 threads load the [ct][rows] tile into LDS in passes of
// PAIR_CTS ct (every load of a pass issued before the first LDS write: 16
// independent loads per thread, each ct a contiguous PAIR_ROWS-value
// segment), then one thread per row folds its column of the tile, the
// accumulator carried across the passes.  (One thread per row walking its CT
// partials alone kept 512 waves on 128 dependent-latency loads each: 0.041 ms
// for cfg2's 17 MB.)
constexpr int PAIR_ROWS = 32, PAIR_CTS = 128;

template <typename T>
__device__ __forceinline__ void finalize_pair_rows(T* tile, const T* rp, i64 CT, i64 R, T* rout, i64 blk) {
  constexpr int LANES = 256 / PAIR_ROWS, LOADS = PAIR_CTS / LANES;
  const int t = threadIdx.x, j = t % PAIR_ROWS, c = t / PAIR_ROWS;
  const i64 r = blk * PAIR_ROWS + j;
  const bool ok = r < R;
  double acc = 0.0;
  for (i64 c0 = 0; c0 < CT; c0 += PAIR_CTS) {
    const int nct = CT - c0 < PAIR_CTS ? (int)(CT - c0) : PAIR_CTS;
    T v[LOADS];
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int ct = c + LANES * i;
      v[i] = (ok && ct < nct) ? rp[(c0 + ct) * R + r] : (T)0;
    }
#pragma unroll
    for (int i = 0; i < LOADS; ++i) tile[(c + LANES * i) * PAIR_ROWS + j] = v[i];
    __syncthreads();
    if (t < PAIR_ROWS) {
      int ct = 0;
      if (c0 == 0) { acc = (double)tile[t]; ct = 1; }
      for (; ct < nct; ++ct) acc += (double)tile[ct * PAIR_ROWS + t];
    }
    __syncthreads();  // the next pass rewrites the tile
  }
  if (t < PAIR_ROWS && ok) rout[r] = (T)acc;
}

__global__ __launch_bounds__(256) void k_finalize_pair(int dt, const void* cpv, i64 P, i64 n, void* cout, int wide,
                                                       unsigned gc, const void* rpv, i64 CT, i64 R, void* rout) {
  if (blockIdx.x < gc) {
    if (wide) finalize_wide(SPX_OP_SUM, dt, dt, cpv, nullptr, P, n, cout, nullptr, blockIdx.x, gc);
    else finalize_thin(SPX_OP_SUM, dt, dt, cpv, nullptr, P, n, cout, nullptr, blockIdx.x, gc);
    return;
  }
  __shared__ double tile[PAIR_CTS * PAIR_ROWS];
  const i64 blk = (i64)(blockIdx.x - gc);
  if (dt == SPX_F32) finalize_pair_rows<float>((float*)tile, (const float*)rpv, CT, R, (float*)rout, blk);
  else finalize_pair_rows<double>(tile, (const double*)rpv, CT, R, (double*)rout, blk);
}

extern "C" int spx_reduce_finalize_pair(int dtype, const void* col_part, int64_t P, int64_t n, void* col_out,
                                        const void* row_part, int64_t CT, int64_t R, void* row_out, void* stream) {
  if (dtype != SPX_F32 && dtype != SPX_F64)
    return set_err(SPX_EINVAL, "spx_reduce_finalize_pair: dtype must be float32 or float64");
  if (P < 1 || n < 0 || CT < 1 || R < 0) return set_err(SPX_EINVAL, "spx_reduce_finalize_pair: bad P/n/CT/R");
  if (n == 0 && R == 0) return SPX_OK;
  if ((n > 0 && (!col_part || !col_out)) || (R > 0 && (!row_part || !row_out)))
    return set_err(SPX_EINVAL, "spx_reduce_finalize_pair: null pointer");
  const unsigned gc = n > 0 ? finalize_grid(P, n) : 0, gr = (unsigned)((R + PAIR_ROWS - 1) / PAIR_ROWS);
  k_finalize_pair<<<gc + gr, 256, 0, S(stream)>>>(dtype, col_part, P, n, col_out, finalize_is_wide(P, n) ? 1 : 0, gc,
                                                  row_part, CT, R, row_out);
  LAUNCH_CHECK("spx_reduce_finalize_pair");
  return SPX_OK;
}

extern "C" int spx_reduce_finalize(int op, int acc_dtype, int out_dtype, const void* part_val,
                                   const int64_t* part_idx, int64_t P, int64_t n, void* out,
                                   void* out_val, void* stream) {
  if (!valid_dtype(acc_dtype) || !valid_dtype(out_dtype))
    return set_err(SPX_EINVAL, "spx_reduce_finalize: bad dtype");
  if (op < SPX_OP_SUM || op > SPX_OP_ARGMAX) return set_err(SPX_EINVAL, "spx_reduce_finalize: bad op %d", op);
  if (P < 1 || n < 0) return set_err(SPX_EINVAL, "spx_reduce_finalize: bad P/n");
  if (n == 0) return SPX_OK;
  if ((op == SPX_OP_ARGMIN || op == SPX_OP_ARGMAX) && !part_idx)
    return set_err(SPX_EINVAL, "spx_reduce_finalize: arg op needs part_idx");
  if (finalize_is_wide(P, n))
    k_finalize_wide<<<finalize_grid(P, n), 256, 0, S(stream)>>>(op, acc_dtype, out_dtype, part_val, part_idx, P, n,
                                                                out, out_val);
  else
    k_finalize<<<finalize_grid(P, n), 256, 0, S(stream)>>>(op, acc_dtype, out_dtype, part_val, part_idx, P, n, out,
                                                           out_val);
  LAUNCH_CHECK("spx_reduce_finalize");
  return SPX_OK;
}

// =================================================================== merge
__global__ __launch_bounds__(256) void k_merge(int op, int dt, void* dst, uint8_t* mask, Geom g,
                                               i64 n, const void* src, int sdt, int fast,
                                               int fast_reduce) {
  // g.a = dst_shape, g.b = region_ul, g.c = region_shape
  i64 stride = (i64)gridDim.x * 256;
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
    i64 di;
    if (fast) {
      di = e;
    } else {
      i64 rem = e, mul = 1;
      di = 0;
      for (int d = g.ndim - 1; d >= 0; --d) {
        i64 li = rem % g.c[d];
        rem /= g.c[d];
        di += (li + g.b[d]) * mul;
        mul *= g.a[d];
      }
    }
    bool reduce;
    if (op == SPX_OP_REPLACE) reduce = false;
    else if (fast) reduce = fast_reduce;
    else reduce = mask ? (mask[di] != 0) : true;
    if (is_float_dt(dt)) {
      double v = ld_f(src, sdt, e);
      if (reduce) v = comb_f(op, ld_f(dst, dt, di), v);
      st_f(dst, dt, di, v);
    } else {
      i64 v = is_float_dt(sdt) ? (i64)ld_f(src, sdt, e) : ld_i(src, sdt, e);
      if (reduce) v = comb_i(op, ld_i(dst, dt, di), v);
      st_i(dst, dt, di, v);
    }
    if (mask) mask[di] = 1;
  }
}

extern "C" int spx_merge(int op, int dtype, void* dst, uint8_t* mask, int ndim,
                         const int64_t* dst_shape, const int64_t* region_ul,
                         const int64_t* region_shape, const void* src, int src_dtype,
                         int full_tile_fastpath, void* stream) {
  if (!valid_dtype(dtype) || !valid_dtype(src_dtype)) return set_err(SPX_EINVAL, "spx_merge: bad dtype");
  if (!(op == SPX_OP_SUM || op == SPX_OP_MIN || op == SPX_OP_MAX || op == SPX_OP_REPLACE))
    return set_err(SPX_EINVAL, "spx_merge: bad op %d", op);
  if (ndim < 0 || ndim > 8) return set_err(SPX_EINVAL, "spx_merge: ndim > 8");
  Geom g{};
  g.ndim = ndim;
  i64 n = 1;
  bool full = true;
  for (int d = 0; d < ndim; ++d) {
    g.a[d] = dst_shape[d];
    g.b[d] = region_ul[d];
    g.c[d] = region_shape[d];
    if (region_ul[d] < 0 || region_ul[d] + region_shape[d] > dst_shape[d])
      return set_err(SPX_EINVAL, "spx_merge: region out of bounds on dim %d", d);
    if (region_ul[d] != 0 || region_shape[d] != dst_shape[d]) full = false;
    n *= region_shape[d];
  }
  if (n == 0) return SPX_OK;
  if (!dst || !src) return set_err(SPX_EINVAL, "spx_merge: null pointer");
  int fast = (full && full_tile_fastpath) ? 1 : 0;
  int fast_reduce = 0;
  if (fast && op != SPX_OP_REPLACE) {
    if (mask) {
      uint8_t m0 = 0;
      HIP_TRY(hipMemcpyAsync(&m0, mask, 1, hipMemcpyDeviceToHost, S(stream)));
      HIP_TRY(hipStreamSynchronize(S(stream)));
      fast_reduce = m0 != 0;
    } else {
      fast_reduce = 1;
    }
  }
  k_merge<<<grid_for(n), 256, 0, S(stream)>>>(op, dtype, dst, mask, g, n, src, src_dtype, fast, fast_reduce);
  LAUNCH_CHECK("spx_merge");
  return SPX_OK;
}

// ============================================================= copy region
struct Geom2 {
  int ndim;
  i64 dshape[8], dul[8], sshape[8], sul[8], cshape[8];
};

__global__ __launch_bounds__(256) void k_copy2(int ddt, void* dst, int sdt, const void* src,
                                               Geom2 g, i64 n) {
  i64 stride = (i64)gridDim.x * 256;
  for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
    i64 rem = e, dm = 1, sm = 1, di = 0, si = 0;
    for (int d = g.ndim - 1; d >= 0; --d) {
      i64 li = rem % g.cshape[d];
      rem /= g.cshape[d];
      di += (li + g.dul[d]) * dm;
      si += (li + g.sul[d]) * sm;
      dm *= g.dshape[d];
      sm *= g.sshape[d];
    }
    if (ddt == sdt) {
      switch (ddt) {
        case SPX_BOOL: ((uint8_t*)dst)[di] = ((const uint8_t*)src)[si]; break;
        case SPX_I32: ((int32_t*)dst)[di] = ((const int32_t*)src)[si]; break;
        case SPX_F32: ((float*)dst)[di] = ((const float*)src)[si]; break;
        case SPX_I64: ((int64_t*)dst)[di] = ((const int64_t*)src)[si]; break;
        default: ((double*)dst)[di] = ((const double*)src)[si]; break;
      }
    } else if (is_float_dt(sdt)) {
      if (is_float_dt(ddt)) st_f(dst, ddt, di, ld_f(src, sdt, si));
      else st_i(dst, ddt, di, (i64)ld_f(src, sdt, si));
    } else {
      st_i(dst, ddt, di, ld_i(src, sdt, si));
    }
  }
}

extern "C" int spx_copy_region(int dst_dtype, void* dst, const int64_t* dst_shape,
                               const int64_t* dst_ul, int src_dtype, const void* src,
                               const int64_t* src_shape, const int64_t* src_ul, int ndim,
                               const int64_t* copy_shape, void* stream) {
  if (!valid_dtype(dst_dtype) || !valid_dtype(src_dtype)) return set_err(SPX_EINVAL, "spx_copy_region: bad dtype");
  if (ndim < 0 || ndim > 8) return set_err(SPX_EINVAL, "spx_copy_region: ndim > 8");
  Geom2 g{};
  g.ndim = ndim;
  i64 n = 1;
  for (int d = 0; d < ndim; ++d) {
    g.dshape[d] = dst_shape[d];
    g.dul[d] = dst_ul[d];
    g.sshape[d] = src_shape[d];
    g.sul[d] = src_ul[d];
    g.cshape[d] = copy_shape[d];
    if (dst_ul[d] < 0 || dst_ul[d] + copy_shape[d] > dst_shape[d] || src_ul[d] < 0 ||
        src_ul[d] + copy_shape[d] > src_shape[d])
      return set_err(SPX_EINVAL, "spx_copy_region: region out of bounds on dim %d", d);
    n *= copy_shape[d];
  }
  if (n == 0) return SPX_OK;
  if (!dst || !src) return set_err(SPX_EINVAL, "spx_copy_region: null pointer");
  k_copy2<<<grid_for(n), 256, 0, S(stream)>>>(dst_dtype, dst, src_dtype, src, g, n);
  LAUNCH_CHECK("spx_copy_region");
  return SPX_OK;
}

// ================================================== arg-reduction combine
__global__ __launch_bounds__(256) void k_argcombine(int op, int dt, const void* vals, const i64* idx,
                                                    i64 R, i64 n, void* out_val, i64* out_idx) {
  i64 stride = (i64)gridDim.x * 256;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    if (is_float_dt(dt)) {
      double b = ld_f(vals, dt, i);
      i64 bi = idx[i];
      for (i64 r = 1; r < R; ++r) arg_fold(op, ld_f(vals, dt, r * n + i), idx[r * n + i], b, bi);
      out_idx[i] = bi;
      if (out_val) st_f(out_val, dt, i, b);
    } else {
      i64 b = ld_i(vals, dt, i);
      i64 bi = idx[i];
      for (i64 r = 1; r < R; ++r) arg_fold(op, ld_i(vals, dt, r * n + i), idx[r * n + i], b, bi);
      out_idx[i] = bi;
      if (out_val) st_i(out_val, dt, i, b);
    }
  }
}

extern "C" int spx_argreduce_combine(int op, int dtype, const void* vals, const int64_t* idx,
                                     int64_t R, int64_t n, void* out_val, int64_t* out_idx,
                                     void* stream) {
  if (op != SPX_OP_ARGMIN && op != SPX_OP_ARGMAX) return set_err(SPX_EINVAL, "spx_argreduce_combine: bad op");
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_argreduce_combine: bad dtype");
  if (R < 1 || n < 0) return set_err(SPX_EINVAL, "spx_argreduce_combine: bad R/n");
  if (n == 0) return SPX_OK;
  if (!vals || !idx || !out_idx) return set_err(SPX_EINVAL, "spx_argreduce_combine: null pointer");
  k_argcombine<<<grid_for(n), 256, 0, S(stream)>>>(op, dtype, vals, idx, R, n, out_val, out_idx);
  LAUNCH_CHECK("spx_argreduce_combine");
  return SPX_OK;
}

// ==================================================================== GEMM
// fp32 / fp64 MFMA kernels live in gemm_kernels.h (shared with the tuning
// harness tools/gemm_tune.hip).  Configurations chosen by measurement on
// MI355X (profiles/r01_gemm_tune.txt):
//   fp32 large: 256x256x16, 16 waves (4x4), grouped order GM=8  -> 136 TF (86.6 %)
//   fp32 small: 128x128x16, 4 waves (2x2), GM=8                 -> 131 TF at 8192
//   fp64      : 128x128x16, 16 waves (4x4)                      -> 69.3 TF (88.2 %)
// (the 4-wave fp64 layout needs 304 registers -> 1 wave per SIMD -> 40 TF).
#include "gemm_kernels.h"

// fp32: 256x128x16, 8 waves (with the k-contiguous A staging: 141.4 TF = 89.9 %
// of 157.3 at 32768^3 against 135.6 TF for the 256x256x16 16-wave tile,
// profiles/r02_gemm_tune_ak.txt)
// fp32: one accumulator set, flushed into C every 512 K-tiles (gemm_kernels.h
// GFL): chains of 4096 MFMA steps instead of K / 2 (four flushes at cfg4's
// K = 32768), at the one-chain form's registers and occupancy (round 3's
// register two-level form, SEG, cost 6 %).  Round 5, the cfg4 product against
// fp64 at EVERY one of its 2^30 elements (tools/gemm_margin.py,
// profiles/r05_gemm_gfl_margin.txt, one box): GFL 1024 141.0 TF, max rel err
// 7.32e-6 (73 % of the 1e-5 budget); 512 140.4 TF, 3.71e-6; 256 140.2 TF,
// 1.80e-6 -- 512 keeps 40 % of the budget in reserve for 0.4 TF
// (test_dot_cfg4_full_size asserts <= 0.6e-5 over all elements).
constexpr int SPX_GEMM_GFL = 512;
typedef spx_mfma::Config<float, 256, 128, 16, 4, 2, 8, 0, SPX_GEMM_GFL> GemmF32Big;
typedef spx_mfma::Config<float, 128, 128, 16, 2, 2, 8, 0, SPX_GEMM_GFL> GemmF32Small;

// C *= beta (the GFL kernels take beta 0 or 1)
__global__ __launch_bounds__(256) void k_scale_rows(i64 M, i64 N, float* C, i64 ldc, float beta) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < M * N; i += (i64)gridDim.x * 256) {
    const i64 r = i / N, c = i % N;
    C[r * ldc + c] *= beta;
  }
}
typedef spx_mfma::Config<double, 128, 128, 16, 4, 4, 0> GemmF64;

// Round 6: the three-stage one-wave-per-SIMD kernels (gemm_kernels.h
// gemm_f32_p3 / gemm_f64_p3) for large aligned products.  fp32: chains of
// SPX_GEMM_GFL K-tiles flushed into C inside the kernel, as the two-stage
// kernel's GFL (the same chains: the cfg4 product is bit-identical to it);
// fp64 (experimental, SPX_GEMM_P3=2): K in launches of SPX_GEMM_KCHUNK.
// SPX_GEMM_P3=0 in the environment selects the two-stage kernels (A/B; read
// once).
constexpr i64 SPX_GEMM_KCHUNK = 8192;
static int gemm_p3_on() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("SPX_GEMM_P3");
    v = e ? atoi(e) : 1;
  }
  return v;
}
template <typename T, typename F>
static hipError_t gemm_kchunks(i64 K, const T* a, const T* b, i64 ldb, T beta, F launch) {
  for (i64 k0 = 0; k0 < K; k0 += SPX_GEMM_KCHUNK) {
    const i64 kc = K - k0 < SPX_GEMM_KCHUNK ? K - k0 : SPX_GEMM_KCHUNK;
    const hipError_t e = launch(kc, a + k0, b + k0 * ldb, k0 ? (T)1 : beta);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// integer GEMM (exact, wrap-around like NumPy's int matmul): 16x16 output
// tile per 256-thread block, K staged through LDS.  Used for integer dot
// products (the reference's tests multiply arange ints); not a hot path.
template <typename T>
__global__ __launch_bounds__(256) void k_gemm_int(i64 M, i64 N, i64 K, const T* __restrict__ A, i64 lda,
                                                  const T* __restrict__ B, i64 ldb, T* __restrict__ C,
                                                  i64 ldc, T alpha, T beta) {
  __shared__ T As[16][17];
  __shared__ T Bs[16][17];
  int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  i64 row = (i64)blockIdx.y * 16 + ty, col = (i64)blockIdx.x * 16 + tx;
  typedef typename std::conditional<sizeof(T) == 8, u64, uint32_t>::type U;
  U acc = 0;
  for (i64 k0 = 0; k0 < K; k0 += 16) {
    As[ty][tx] = (row < M && k0 + tx < K) ? A[row * lda + k0 + tx] : (T)0;
    Bs[ty][tx] = (k0 + ty < K && col < N) ? B[(k0 + ty) * ldb + col] : (T)0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) acc += (U)As[ty][k] * (U)Bs[k][tx];
    __syncthreads();
  }
  if (row < M && col < N) {
    U v = (U)alpha * acc;
    if (beta != 0) v += (U)beta * (U)C[row * ldc + col];
    C[row * ldc + col] = (T)v;
  }
}

// The route of a product: which kernel, which instantiation, its block tile
// and the K distance between its flushes into C.  Pure host code -- A and B
// are looked at for their address bits only -- shared by spx_gemm and
// spx_gemm_plan, so what the plan answers is what the call launches.
struct GemmRoute {
  int kernel = SPX_GEMM_NONE;
  bool aligned = false;
  int bm = 0, bn = 0, bk = 0;
  i64 flush_k = 0;
};
// the argument checks of spx_gemm in its order (C and ldc only for the call
// itself: with_c), then the selection; route.kernel stays SPX_GEMM_NONE where
// there is nothing to launch (M == 0 or N == 0)
static int gemm_route(const char* who, int dtype, i64 M, i64 N, i64 K, const void* A, i64 lda, const void* B, i64 ldb,
                      bool with_c, const void* C, i64 ldc, GemmRoute& r) {
  if (dtype != SPX_F32 && dtype != SPX_F64 && dtype != SPX_I32 && dtype != SPX_I64)
    return set_err(SPX_ENOTSUP, "%s: dtype %d not supported (F32/F64/I32/I64)", who, dtype);
  if (M < 0 || N < 0 || K < 0) return set_err(SPX_EINVAL, "%s: negative dimension", who);
  if (lda < K || ldb < N || (with_c && ldc < N)) return set_err(SPX_EINVAL, "%s: leading dimension too small", who);
  if (M == 0 || N == 0) return SPX_OK;
  if (!A || !B || (with_c && !C)) return set_err(SPX_EINVAL, "%s: null pointer", who);
  if (K == 0) {  // C = beta * C
    return set_err(SPX_ENOTSUP, "%s: K == 0 not supported", who);
  }
  auto set = [&](int kernel, bool aligned, int bm, int bn, int bk, i64 flush_k) {
    r.kernel = kernel, r.aligned = aligned, r.bm = bm, r.bn = bn, r.bk = bk, r.flush_k = flush_k;
  };
  if (dtype == SPX_I32 || dtype == SPX_I64) {
    set(SPX_GEMM_INT, false, 16, 16, 16, 0);
  } else if (dtype == SPX_F32) {
    i64 big_tiles = ((M + 255) / 256) * ((N + 255) / 256);
    if (big_tiles >= 512 && big_tiles <= 0x7fffffffLL && gemm_p3_on() && spx_mfma::p3_ok(M, N, K, A, lda, B, ldb)) {
      set(SPX_GEMM_F32_P3, true, 256, 256, 16, (i64)SPX_GEMM_GFL * 16);
    } else if (big_tiles >= 512) {
      if (big_tiles > 0x7fffffffLL) return set_err(SPX_EINVAL, "%s: too many tiles", who);
      set(SPX_GEMM_F32_BIG, GemmF32Big::is_aligned(M, N, K, A, lda, B, ldb), GemmF32Big::bm, GemmF32Big::bn,
          GemmF32Big::bk, (i64)SPX_GEMM_GFL * GemmF32Big::bk);
    } else {
      set(SPX_GEMM_F32_SMALL, GemmF32Small::is_aligned(M, N, K, A, lda, B, ldb), GemmF32Small::bm, GemmF32Small::bn,
          GemmF32Small::bk, (i64)SPX_GEMM_GFL * GemmF32Small::bk);
    }
  } else {
    i64 tiles = ((M + 127) / 128) * ((N + 127) / 128);
    if (tiles > 0x7fffffffLL) return set_err(SPX_EINVAL, "%s: too many tiles", who);
    if (tiles >= 1024 && gemm_p3_on() > 1 && spx_mfma::p3d_ok<16>(M, N, K, A, lda, B, ldb))
      set(SPX_GEMM_F64_P3, true, 128, 128, 16, SPX_GEMM_KCHUNK);
    else
      set(SPX_GEMM_F64, GemmF64::is_aligned(M, N, K, A, lda, B, ldb), GemmF64::bm, GemmF64::bn, GemmF64::bk, 0);
  }
  return SPX_OK;
}

extern "C" int spx_gemm_plan(int dtype, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                             int64_t ldb, int64_t* kernel, int64_t* aligned, int64_t* bm, int64_t* bn, int64_t* bk,
                             int64_t* flush_k) {
  GemmRoute r;
  const int rc = gemm_route("spx_gemm_plan", dtype, M, N, K, A, lda, B, ldb, false, nullptr, 0, r);
  if (rc != SPX_OK) return rc;
  if (kernel) *kernel = r.kernel;
  if (aligned) *aligned = r.aligned ? 1 : 0;
  if (bm) *bm = r.bm;
  if (bn) *bn = r.bn;
  if (bk) *bk = r.bk;
  if (flush_k) *flush_k = r.flush_k;
  return SPX_OK;
}

extern "C" int spx_gemm(int dtype, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
                        const void* B, int64_t ldb, void* C, int64_t ldc, double alpha,
                        double beta, void* stream) {
  GemmRoute r;
  const int rc = gemm_route("spx_gemm", dtype, M, N, K, A, lda, B, ldb, true, C, ldc, r);
  if (rc != SPX_OK || r.kernel == SPX_GEMM_NONE) return rc;
  if (r.kernel == SPX_GEMM_INT) {
    dim3 grid((unsigned)((N + 15) / 16), (unsigned)((M + 15) / 16));
    if (dtype == SPX_I64)
      k_gemm_int<int64_t><<<grid, 256, 0, S(stream)>>>(M, N, K, (const int64_t*)A, lda, (const int64_t*)B, ldb,
                                                       (int64_t*)C, ldc, (int64_t)alpha, (int64_t)beta);
    else
      k_gemm_int<int32_t><<<grid, 256, 0, S(stream)>>>(M, N, K, (const int32_t*)A, lda, (const int32_t*)B, ldb,
                                                       (int32_t*)C, ldc, (int32_t)alpha, (int32_t)beta);
    LAUNCH_CHECK("spx_gemm(int)");
    return SPX_OK;
  }
  hipError_t e;
  if (dtype == SPX_F32) {
    const float *a = (const float*)A, *b = (const float*)B;
    if (beta != 0.0 && beta != 1.0) {
      k_scale_rows<<<(unsigned)std::min<i64>((M * N + 255) / 256, 4096), 256, 0, S(stream)>>>(M, N, (float*)C, ldc,
                                                                                           (float)beta);
      LAUNCH_CHECK("spx_gemm(scale C)");
      beta = 1.0;
    }
    if (r.kernel == SPX_GEMM_F32_P3) {
      // one launch, K in chunks of SPX_GEMM_GFL K-tiles inside the kernel
      // (beta is 0 or 1 here, as the flush needs)
      e = spx_mfma::p3_launch<8, 0, SPX_GEMM_GFL, 1, 4>(M, N, K, a, lda, b, ldb, (float*)C, ldc, (float)alpha,
                                                         (float)beta, S(stream));
    } else if (r.kernel == SPX_GEMM_F32_BIG) {
      e = GemmF32Big::launch(M, N, K, a, lda, b, ldb, (float*)C, ldc, (float)alpha, (float)beta, r.aligned,
                             S(stream));
    } else {
      e = GemmF32Small::launch(M, N, K, a, lda, b, ldb, (float*)C, ldc, (float)alpha, (float)beta, r.aligned,
                               S(stream));
    }
    if (e != hipSuccess) return set_err(SPX_EHIP, "spx_gemm(f32) launch failed: %s", hipGetErrorString(e));
  } else {
    const double *a = (const double*)A, *b = (const double*)B;
    if (r.kernel == SPX_GEMM_F64_P3) {
      e = gemm_kchunks<double>(K, a, b, ldb, beta, [&](i64 kc, const double* ak, const double* bk, double bt) {
        return spx_mfma::p3d_launch<8, 16, 0, 4>(M, N, kc, ak, lda, bk, ldb, (double*)C, ldc, alpha, bt, S(stream));
      });
    } else {
      e = GemmF64::launch(M, N, K, a, lda, b, ldb, (double*)C, ldc, alpha, beta, r.aligned, S(stream));
    }
    if (e != hipSuccess) return set_err(SPX_EHIP, "spx_gemm(f64) launch failed: %s", hipGetErrorString(e));
  }
  return SPX_OK;
}

// ================================================================ k-means
#include "kmeans_kernels.h"

// ============================================================ prefix scan
#include "scan_kernels.h"

// ========================================================= sort / argsort
#include "sort_kernels.h"

// ================================================= topk / nearest neighbours
#include "topk_kernels.h"

// ========================================================= take / compress
#include "index_kernels.h"

// ===================================================== stencil / maxpool
#include "stencil_kernels.h"

// ============================================ cholesky / triangular solve
#include "linalg_kernels.h"

// ================================================= Householder TSQR (qr)
#include "qr_kernels.h"

// ===================================== batched Jacobi eigen-solver (eigh)
#include "eigh_kernels.h"

// ============================= batched one-sided Jacobi SVD (svd / pinv)
#include "svd_kernels.h"

// ============================================== sparse (CSR) x dense, todense
#include "sparse_kernels.h"

// ===================================== alternating least squares (row solves)
#include "als_kernels.h"

// ============================== all-pairs shortest paths (Floyd-Warshall)
#include "graph_kernels.h"

// ================================ fuzzy k-means (fused soft-assignment step)
#include "fuzzy_kernels.h"

// ======================================== n-body (all-pairs direct summation)
#include "nbody_kernels.h"

// ============================ pairwise kernels (affinity matrix, row degrees)
#include "affinity_kernels.h"

// ============================================================ JIT modules
extern "C" int spx_module_load(const void* image, size_t nbytes, void** module_out) {
  if (!image || nbytes == 0 || !module_out) return set_err(SPX_EINVAL, "spx_module_load: bad args");
  hipModule_t m = nullptr;
  HIP_TRY(hipModuleLoadData(&m, image));
  *module_out = (void*)m;
  return SPX_OK;
}

extern "C" int spx_module_unload(void* module) {
  if (!module) return SPX_OK;
  HIP_TRY(hipModuleUnload((hipModule_t)module));
  return SPX_OK;
}

extern "C" int spx_module_function(void* module, const char* name, void** fn_out) {
  if (!module || !name || !fn_out) return set_err(SPX_EINVAL, "spx_module_function: bad args");
  hipFunction_t f = nullptr;
  hipError_t e = hipModuleGetFunction(&f, (hipModule_t)module, name);
  if (e != hipSuccess)
    return set_err(SPX_EHIP, "hipModuleGetFunction(%s): %s", name, hipGetErrorString(e));
  *fn_out = (void*)f;
  return SPX_OK;
}

extern "C" int spx_launch(void* fn, uint32_t gx, uint32_t gy, uint32_t gz, uint32_t block_x,
                          uint32_t shared_bytes, const void* args, size_t args_bytes, void* stream) {
  if (!fn) return set_err(SPX_EINVAL, "spx_launch: null function");
  if (gx == 0 || gy == 0 || gz == 0) return SPX_OK;
  if (block_x == 0 || block_x > 1024) return set_err(SPX_EINVAL, "spx_launch: bad block %u", block_x);
  size_t sz = args_bytes;
  void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, const_cast<void*>(args), HIP_LAUNCH_PARAM_BUFFER_SIZE,
                 &sz, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel((hipFunction_t)fn, gx, gy, gz, block_x, 1, 1, shared_bytes, S(stream),
                                nullptr, cfg));
  return SPX_OK;
}

// als_kernels.h -- the per-row normal-equation solve of alternating least
// squares (spx_als_solve) for gfx950.  Included from spx.hip.
//
// For every row i of the CSR matrix A (m x n) with K_i = { k : val[k] != 0 }:
//
//   G_i = sum_{k in K_i} y_{col[k]} y_{col[k]}^T + lambda |K_i| I      (f x f)
//   b_i = sum_{k in K_i} val[k] y_{col[k]}
//   X[i, :] = G_i^{-1} b_i          (Cholesky, forward and back substitution)
//
// One wave owns a row, ALS_ROWS waves make a 256-thread workgroup.  Lane p < f
// holds row p of G_i (FB >= f doubles, FB the register bucket of f) and b_p in
// registers.  Per nonzero the wave reads the gathered Y row once -- lane p
// loads Y[col, p], f adjacent elements -- parks it as doubles in its LDS strip
// and every lane reads it back with broadcast reads; the next Y row is loaded
// while the current one is consumed, and the park buffer is double, so one
// wave barrier per nonzero is enough.  The nonzeros of a row are walked in
// stored order by the one wave: every entry of G_i and b_i is one serial sum.
//
// The factorization runs in the wave's strip: G_i is stored with the odd row
// stride f | 1 (lane p at row p: distinct banks), factored right-looking column
// by column, and the two substitutions keep the right-hand side in registers
// and pass the pivot element by a wave shuffle.  Everything is float64 for
// both dtypes; T only says what is loaded and stored.
//
// No float atomics, and no value depends on anything but the row's own entries,
// Y, f, lambda and T.  A pivot that is not positive and finite ends the row:
// it is filled with NaN and *info is incremented (an integer atomic).
//
// The strip is f (f | 1) + 2 * 64 doubles: 34304 bytes at f = 64, 137216 for the
// four waves of a workgroup, inside the 160 KiB of a CU.
#pragma once

namespace spx_als {

constexpr int FMAX = 64;
constexpr int ALS_ROWS = 4;  // rows (waves) per workgroup
constexpr int BLOCK = 64 * ALS_ROWS;
constexpr int MAX_GRID = 1 << 20;

static inline i64 strip_doubles(i64 f) { return f * (f | 1) + 2 * FMAX; }

__device__ __forceinline__ void wave_sync() {
  // the lanes of a wave run in step, and a wave's LDS operations complete in
  // issue order: what is needed is that the compiler keeps them in order
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T, int FB>
__global__ __launch_bounds__(BLOCK) void k_als_solve(i64 m, int f, i64 nnz, const i64* __restrict__ rowptr,
                                                     const int32_t* __restrict__ col, const T* __restrict__ val,
                                                     const T* __restrict__ Y, i64 ldy, double lambda,
                                                     T* __restrict__ X, i64 ldx, int32_t* info, i64 strip) {
  extern __shared__ __attribute__((aligned(16))) unsigned char als_smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* G = (double*)als_smem + (i64)wave * strip;
  const int ld = f | 1;
  double* park = G + (i64)f * ld;  // 2 x 64 doubles
  const bool mine = lane < f;

  for (i64 i = (i64)blockIdx.x * ALS_ROWS + wave; i < m; i += (i64)gridDim.x * ALS_ROWS) {  // uniform over the wave
    i64 s = rowptr[i], e = rowptr[i + 1];
    if (s < 0) s = 0;  // a malformed rowptr: never outside col / val
    if (e > nnz) e = nnz;

    double g[FB];
#pragma unroll
    for (int q = 0; q < FB; ++q) g[q] = 0.0;
    double b = 0.0;
    i64 cnt = 0;

    // the first counted entry
    i64 k = s;
    while (k < e && val[k] == (T)0) ++k;
    double v = 0.0, y = 0.0;
    if (k < e) {
      v = (double)val[k];
      y = mine ? (double)Y[(i64)col[k] * ldy + lane] : 0.0;
    }
    int buf = 0;
    while (k < e) {
      park[buf * FMAX + lane] = y;
      // the next counted entry, loaded while this one is consumed
      i64 kn = k + 1;
      while (kn < e && val[kn] == (T)0) ++kn;
      double vn = 0.0, yn = 0.0;
      if (kn < e) {
        vn = (double)val[kn];
        yn = mine ? (double)Y[(i64)col[kn] * ldy + lane] : 0.0;
      }
      wave_sync();
      const double* yr = park + buf * FMAX;
#pragma unroll
      for (int q = 0; q < FB; ++q) g[q] += y * yr[q];
      b += v * y;
      ++cnt;
      k = kn;
      v = vn;
      y = yn;
      buf ^= 1;
    }

    if (cnt == 0) {  // lstsq of the zero system
      if (mine) X[i * ldx + lane] = (T)0;
      continue;
    }

    // G into the strip (the lower triangle is what the factorization reads)
    wave_sync();
    if (mine) {
#pragma unroll
      for (int q = 0; q < FB; ++q)
        if (q < f) G[lane * ld + q] = g[q];
    }
    wave_sync();
    if (mine) G[lane * ld + lane] += lambda * (double)cnt;
    wave_sync();

    // right-looking Cholesky, G = L L^T, L in the lower triangle
    bool ok = true;
    for (int j = 0; j < f; ++j) {
      const double d = G[j * ld + j];  // the same word for every lane
      if (!(d > 0.0) || d > 1.79769313486231570e308) {
        ok = false;
        break;
      }
      const double r = sqrt(d);
      double l = 0.0;
      if (lane > j && mine) {
        l = G[lane * ld + j] / r;
        G[lane * ld + j] = l;
      }
      if (lane == j) G[j * ld + j] = r;
      wave_sync();
      if (lane > j && mine) {
        // eight words at a time, all loads before the stores: a row word (column > j) is never a word of
        // column j, and the loop is bound by LDS latency, not by its arithmetic
        double* row = G + lane * ld;
        const double* cj = G + j;
        int q = j + 1;
        for (; q + 7 <= lane; q += 8) {
          double c[8], r[8];
#pragma unroll
          for (int t = 0; t < 8; ++t) c[t] = cj[(q + t) * ld];
#pragma unroll
          for (int t = 0; t < 8; ++t) r[t] = row[q + t];
#pragma unroll
          for (int t = 0; t < 8; ++t) row[q + t] = r[t] - l * c[t];
        }
        for (; q <= lane; ++q) row[q] -= l * cj[q * ld];
      }
      wave_sync();
    }
    if (!ok) {
      if (mine) X[i * ldx + lane] = (T)__builtin_nan("");
      if (lane == 0) atomicAdd(info, 1);
      continue;
    }

    // L z = b, then L^T x = z: the right-hand side stays in the lanes
    for (int j = 0; j < f; ++j) {
      if (lane == j) b = b / G[j * ld + j];
      const double z = __shfl(b, j);
      if (lane > j && mine) b -= G[lane * ld + j] * z;
    }
    for (int j = f - 1; j >= 0; --j) {
      if (lane == j) b = b / G[j * ld + j];
      const double x = __shfl(b, j);
      if (lane < j) b -= G[j * ld + lane] * x;
    }
    if (mine) X[i * ldx + lane] = (T)b;
    wave_sync();  // the strip is the next row's
  }
}

template <typename T, int FB>
static hipError_t launch(i64 m, i64 f, i64 nnz, const i64* rowptr, const int32_t* col, const T* val, const T* Y,
                         i64 ldy, double lambda, T* X, i64 ldx, int32_t* info, hipStream_t s) {
  const i64 strip = strip_doubles(f);
  const size_t lds = (size_t)(strip * ALS_ROWS * (i64)sizeof(double));
  hipError_t e = hipFuncSetAttribute((const void*)k_als_solve<T, FB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds);
  if (e != hipSuccess) return e;
  const i64 blocks = (m + ALS_ROWS - 1) / ALS_ROWS;
  hipLaunchKernelGGL((k_als_solve<T, FB>), dim3((unsigned)std::min<i64>(blocks, MAX_GRID)), dim3(BLOCK), lds, s, m,
                     (int)f, nnz, rowptr, col, val, Y, ldy, lambda, X, ldx, info, strip);
  return hipGetLastError();
}

template <typename T>
static hipError_t run(i64 m, i64 f, i64 nnz, const i64* rowptr, const int32_t* col, const T* val, const T* Y, i64 ldy,
                      double lambda, T* X, i64 ldx, int32_t* info, hipStream_t s) {
  hipError_t e = hipMemsetAsync(info, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  if (f <= 8) return launch<T, 8>(m, f, nnz, rowptr, col, val, Y, ldy, lambda, X, ldx, info, s);
  if (f <= 16) return launch<T, 16>(m, f, nnz, rowptr, col, val, Y, ldy, lambda, X, ldx, info, s);
  if (f <= 32) return launch<T, 32>(m, f, nnz, rowptr, col, val, Y, ldy, lambda, X, ldx, info, s);
  return launch<T, 64>(m, f, nnz, rowptr, col, val, Y, ldy, lambda, X, ldx, info, s);
}

}  // namespace spx_als

// ------------------------------------------------------------------ C ABI
extern "C" int spx_als_plan(int dtype, int64_t f, int64_t* fmax, int64_t* rows_per_block) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_als_plan: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_als_plan: dtype %d is not float32 / float64", dtype);
  if (f < 0) return set_err(SPX_EINVAL, "spx_als_plan: negative size (f %lld)", (long long)f);
  if (fmax) *fmax = spx_als::FMAX;
  if (rows_per_block) *rows_per_block = f >= 1 && f <= spx_als::FMAX ? spx_als::ALS_ROWS : 0;
  return SPX_OK;
}

extern "C" int spx_als_solve(int dtype, int64_t m, int64_t n, int64_t f, int64_t nnz, const int64_t* rowptr,
                             const int32_t* col, const void* val, const void* Y, int64_t ldy, double lambda, void* X,
                             int64_t ldx, int32_t* info, void* stream) {
  int rc = sp_check("spx_als_solve", dtype, m, nnz, f);
  if (rc != SPX_OK) return rc;
  if (n < 0) return set_err(SPX_EINVAL, "spx_als_solve: negative size (n %lld)", (long long)n);
  if (n > 0x7fffffffLL)
    return set_err(SPX_ENOTSUP, "spx_als_solve: n = %lld is above the int32 column range", (long long)n);
  if (f < 1) return set_err(SPX_EINVAL, "spx_als_solve: f = %lld is below 1", (long long)f);
  if (f > spx_als::FMAX)
    return set_err(SPX_ENOTSUP, "spx_als_solve: f = %lld is above fmax = %d", (long long)f, spx_als::FMAX);
  if (ldy < f || ldx < f)
    return set_err(SPX_EINVAL, "spx_als_solve: leading dimension (ldy %lld, ldx %lld) below f = %lld", (long long)ldy,
                   (long long)ldx, (long long)f);
  if (!(lambda >= 0.0) || !std::isfinite(lambda))
    return set_err(SPX_EINVAL, "spx_als_solve: lambda = %g is not finite and non-negative", lambda);
  if (m == 0) return SPX_OK;
  if (!rowptr || !X || !info) return set_err(SPX_EINVAL, "spx_als_solve: null rowptr / X / info");
  if (nnz > 0 && (!col || !val || !Y)) return set_err(SPX_EINVAL, "spx_als_solve: null col / val / Y with nnz > 0");
  if (X == Y) return set_err(SPX_EINVAL, "spx_als_solve: X may not alias Y");
  hipError_t e = dtype == SPX_F32
                     ? spx_als::run<float>(m, f, nnz, rowptr, col, (const float*)val, (const float*)Y, ldy, lambda,
                                           (float*)X, ldx, info, S(stream))
                     : spx_als::run<double>(m, f, nnz, rowptr, col, (const double*)val, (const double*)Y, ldy, lambda,
                                            (double*)X, ldx, info, S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_als_solve failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

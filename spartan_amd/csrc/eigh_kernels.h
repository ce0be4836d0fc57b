// Batched symmetric eigen-solver: spx_syevj_plan / spx_syevj.
// Included from spx.hip after qr_kernels.h.
//
// All eigenvalues and eigenvectors of `batch` symmetric n x n matrices
// (n <= nmax) by the parallel cyclic Jacobi method: ONE workgroup per matrix,
// the grid over the batch, nothing but the load and the final store touches
// global memory.
//
// LDS: A (mirrored to the full symmetric matrix at load) and V (the identity
// at the start), both column-major with the odd stride RS = n + 1 -- the lanes
// walk a column at unit stride (the column phase) and a row at stride RS (the
// row phase), both without a bank conflict, the layout argument of
// qr_kernels.h --, the round's table (c, s, a_pp', a_qq' per pair), the
// finish's permutation and one flag word.
//
// Preparation: the largest magnitude of the named triangle decides the case --
// zero (W = 0, V = I, info = 0), not finite (NaN outputs, info = -1), else the
// matrix is scaled by that magnitude's power of two (exact), so that no square
// or quotient below overflows.  tau = u ||A||_F / n, the sum accumulated in
// double in a fixed order.
//
// A sweep is m - 1 rounds of the round-robin tournament over m = n + (n & 1)
// indices: index m - 1 stays, the others rotate; round r pairs (m - 1, r) and
// (r + k, r - k) mod (m - 1), k = 1 .. m / 2 - 1.  The m / 2 pairs of a round
// are disjoint and a sweep meets every pair exactly once; for odd n the pair
// with the phantom index n idles.  A round: one thread per pair forms the
// rotation (Rutishauser's formulas, true divisions) where |a_pq| > tau and sets
// the flag; barrier; columns p, q of A and of V are rotated; barrier; rows p, q
// of A are rotated and a_pp, a_qq, a_pq = a_qp = 0 written exactly; barrier.
// A sweep whose flag stayed clear ends the iteration; every thread takes that
// decision from the same LDS word after a barrier, and the flag's reset is
// separated from the read by another barrier.  SWEEP_MAX bounds the loop.
//
// Finish: w_j = ldexp(a_jj, e); the rank of w_j is the count of the w_i that
// sort before it (ties by index: stable, ascending, no sort); column j of V goes
// to its rank's column with the sign that makes its entry of largest magnitude
// (the first on a tie) positive.
//
// The workgroup size depends on n alone and no atomics are used: a matrix's
// result is the same bits wherever it stands in a batch.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

namespace spx_eigh {

typedef int64_t i64;

constexpr int SWEEP_MAX = 64;
constexpr int MAX_WAVES = 16;
constexpr i64 LDS_BYTES = 160 * 1024;  // what one workgroup may declare

// The one statement of the LDS layout: MAX_WAVES doubles of reduction scratch,
// A and V (n columns of n + 1 each), the table (4 numbers for each of the m / 2
// pairs; the finish keeps w and the signs there: 2 m >= 2 n), the inverse of
// the ranks (n ints), the flag word (padded to 16 bytes).
__host__ __device__ inline size_t lds_bytes(int esize, i64 n) {
  const i64 m = n + (n & 1);
  return (size_t)MAX_WAVES * 8 + (size_t)(2 * n * (n + 1) + 2 * m) * esize + (size_t)n * 4 + 16;
}

// The largest multiple of 32 whose layout fits: 128 (float32), 96 (float64).
inline i64 nmax_of(int esize) {
  i64 n = 32;
  while (lds_bytes(esize, n + 32) <= (size_t)LDS_BYTES) n += 32;
  return n;
}

// Workgroup size from n alone: a small matrix takes little LDS and few waves,
// so that several workgroups share a CU; a large one fills the LDS of its CU
// and takes 8 / 16 waves, because the two phases are bound by the rate of
// 4-byte LDS loads and stores, which one CU reaches only with several waves on
// every SIMD (measured: 16 waves are 1.6 x faster than 8 at n = 128).
inline int threads_of(i64 n) { return n <= 16 ? 64 : n <= 32 ? 128 : n <= 64 ? 512 : 1024; }

template <typename T>
struct Eps;
template <>
struct Eps<float> {
  static constexpr double u = 5.9604644775390625e-08;  // 2^-24
};
template <>
struct Eps<double> {
  static constexpr double u = 1.1102230246251565e-16;  // 2^-53
};

// Pair k of round r over m indices (m even), p < q.  q == n marks the phantom.
__device__ inline void pair_of(int k, int r, int m, int& p, int& q) {
  int x, y;
  if (k == 0) {
    x = m - 1;
    y = r;
  } else {
    x = r + k;
    if (x >= m - 1) x -= m - 1;
    y = r - k;
    if (y < 0) y += m - 1;
  }
  p = x < y ? x : y;
  q = x < y ? y : x;
}

template <typename T>
__device__ inline void fill_nan(T* __restrict__ Wb, T* __restrict__ Vb, i64 ldv, int n, int tid, int nt) {
  const T nan = std::numeric_limits<T>::quiet_NaN();
  for (int j = tid; j < n; j += nt) Wb[j] = nan;
  for (int idx = tid; idx < n * n; idx += nt) {
    const int i = idx / n, c = idx - i * n;
    Vb[(i64)i * ldv + c] = nan;
  }
}

template <typename T>
__global__ __launch_bounds__(1024) void k_syevj(int uplo, int n, int lr_log2, const T* __restrict__ A, i64 lda,
                                               i64 stride_a, T* __restrict__ W, i64 stride_w, T* __restrict__ V,
                                               i64 ldv, i64 stride_v, int32_t* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) unsigned char eigh_smem[];
  const int RS = n + 1, m = n + (n & 1), npairs = m >> 1;
  double* red = (double*)eigh_smem;
  T* a = (T*)(red + MAX_WAVES);
  T* v = a + n * RS;
  T* tab = v + n * RS;
  int* inv = (int*)(tab + 4 * npairs);
  int* flag = inv + n;
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  // LR = 2^lr_log2 lanes walk one column (or row); the workgroup is nt / LR such groups
  const int LR = 1 << lr_log2, sub = tid & (LR - 1), grp = tid >> lr_log2, ngroups = nt >> lr_log2;
  const i64 b = blockIdx.x;
  const T* Ab = A + b * stride_a;
  T* Wb = W + b * stride_w;
  T* Vb = V + b * stride_v;

  // ---- load: mirror the triangle, V = I, the largest magnitude (inf: not finite)
  T amax = 0;
  for (int idx = tid; idx < n * n; idx += nt) {
    const int i = idx / n, j = idx - i * n;
    v[j * RS + i] = i == j ? (T)1 : (T)0;
    if (uplo == 0 ? j <= i : j >= i) {
      const T x = Ab[(i64)i * lda + j];
      a[j * RS + i] = x;
      a[i * RS + j] = x;
      const T ax = fabs(x);
      amax = fmax(amax, ax <= std::numeric_limits<T>::max() ? ax : std::numeric_limits<T>::infinity());
    }
  }
  for (int j = tid; j < n; j += nt) {
    a[j * RS + n] = 0;  // the pad of each column: never used, but summed below
    inv[j] = j;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o, 64));
  if (lane == 0) red[wave] = (double)amax;
  __syncthreads();
  double big = 0;
  for (int w = 0; w < nw; ++w) big = fmax(big, red[w]);
  __syncthreads();  // red is used again
  if (big == 0) {   // (uniform: every thread read the same words)
    for (int j = tid; j < n; j += nt) Wb[j] = 0;
    for (int idx = tid; idx < n * n; idx += nt) {
      const int i = idx / n, c = idx - i * n;
      Vb[(i64)i * ldv + c] = i == c ? (T)1 : (T)0;
    }
    if (tid == 0) info[b] = 0;
    return;
  }
  if (!(big <= (double)std::numeric_limits<T>::max())) {
    fill_nan(Wb, Vb, ldv, n, tid, nt);
    if (tid == 0) info[b] = -1;
    return;
  }

  // ---- scale by the power of two of the largest magnitude; tau = u ||A||_F / n
  const int e = ilogb((T)big);
  double ss = 0;
  for (int idx = tid; idx < n * RS; idx += nt) {
    const T x = ldexp(a[idx], -e);
    a[idx] = x;
    ss += (double)x * (double)x;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) red[wave] = ss;
  __syncthreads();
  ss = 0;
  for (int w = 0; w < nw; ++w) ss += red[w];
  const T tau = (T)(Eps<T>::u * sqrt(ss) / (double)n);

  // ---- the sweeps
  int sweeps = 0;
  bool converged = n == 1;  // no pair: nothing to do
  if (n > 1) {
    for (int sweep = 0; sweep < SWEEP_MAX; ++sweep) {
      if (tid == 0) flag[0] = 0;
      __syncthreads();  // the reset, before any round sets the flag
      for (int r = 0; r < m - 1; ++r) {
        if (tid < npairs) {
          int p, q;
          pair_of(tid, r, m, p, q);
          T c = 1, s = 0, npp = 0, nqq = 0;
          if (q < n) {
            const T apq = a[q * RS + p];
            if (fabs(apq) > tau) {
              const T app = a[p * RS + p], aqq = a[q * RS + q];
              const T theta = (aqq - app) / (2 * apq);
              T t = 1 / (fabs(theta) + sqrt(theta * theta + 1));
              if (theta < 0) t = -t;
              c = 1 / sqrt(t * t + 1);
              s = t * c;
              npp = app - t * apq;
              nqq = aqq + t * apq;
              flag[0] = 1;  // a plain store of the same value by every rotating pair
            }
          }
          tab[4 * tid] = c;
          tab[4 * tid + 1] = s;
          tab[4 * tid + 2] = npp;
          tab[4 * tid + 3] = nqq;
        }
        __syncthreads();
        // column phase: columns p, q of A (even work items) and of V (odd ones)
        for (int w = grp; w < 2 * npairs; w += ngroups) {
          const int k = w >> 1;
          const T c = tab[4 * k], s = tab[4 * k + 1];
          if (s == 0) continue;  // no rotation (the phantom's pair included)
          int p, q;
          pair_of(k, r, m, p, q);
          T* base = (w & 1) ? v : a;
          T* xp = base + p * RS;
          T* xq = base + q * RS;
          for (int i = sub; i < n; i += LR) {
            const T x = xp[i], y = xq[i];
            xp[i] = c * x - s * y;
            xq[i] = s * x + c * y;
          }
        }
        __syncthreads();
        // row phase: rows p, q of A; the 2 x 2 block is written exactly
        for (int k = grp; k < npairs; k += ngroups) {
          const T c = tab[4 * k], s = tab[4 * k + 1];
          if (s == 0) continue;
          const T npp = tab[4 * k + 2], nqq = tab[4 * k + 3];
          int p, q;
          pair_of(k, r, m, p, q);
          for (int j = sub; j < n; j += LR) {
            T* col = a + j * RS;
            const T x = col[p], y = col[q];
            T nx = c * x - s * y, ny = s * x + c * y;
            if (j == p) {
              nx = npp;
              ny = 0;
            } else if (j == q) {
              nx = 0;
              ny = nqq;
            }
            col[p] = nx;
            col[q] = ny;
          }
        }
        __syncthreads();
      }
      const int rotated = flag[0];  // after the round's last barrier: the same word for every thread
      __syncthreads();              // this read, before the next sweep's reset
      sweeps = sweep + 1;
      if (!rotated) {
        converged = true;
        break;
      }
    }
  }
  if (!converged) {
    fill_nan(Wb, Vb, ldv, n, tid, nt);
    if (tid == 0) info[b] = -1;
    return;
  }

  // ---- finish: eigenvalues, ranks, signs, the permuted store
  T* w = tab;
  T* sg = tab + n;
  __syncthreads();
  for (int j = tid; j < n; j += nt) w[j] = ldexp(a[j * RS + j], e);
  __syncthreads();
  for (int j = tid; j < n; j += nt) {
    const T wj = w[j];
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
      const T wi = w[i];
      cnt += (wi < wj || (wi == wj && i < j)) ? 1 : 0;
    }
    inv[cnt] = j;
    Wb[cnt] = wj;
    const T* col = v + j * RS;
    T best = 0;
    bool neg = false;
    for (int i = 0; i < n; ++i) {
      const T x = col[i], ax = fabs(x);
      if (ax > best) {
        best = ax;
        neg = x < 0;
      }
    }
    sg[j] = neg ? (T)-1 : (T)1;
  }
  __syncthreads();
  for (int idx = tid; idx < n * n; idx += nt) {
    const int i = idx / n, c = idx - i * n;
    const int j = inv[c];
    Vb[(i64)i * ldv + c] = sg[j] * v[j * RS + i];
  }
  if (tid == 0) info[b] = sweeps;
}

template <typename T>
static hipError_t run(int uplo, i64 batch, i64 n, const T* A, i64 lda, i64 stride_a, T* W, i64 stride_w, T* V, i64 ldv,
                      i64 stride_v, int32_t* info, hipStream_t s) {
  const size_t lds = lds_bytes(sizeof(T), n);
  const int nt = threads_of(n);
  int lr = 0;
  while ((1 << lr) < n && lr < 6) ++lr;
  hipError_t e = hipFuncSetAttribute((const void*)k_syevj<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_syevj<T>), dim3((unsigned)batch), dim3(nt), lds, s, uplo, (int)n, lr, A, lda, stride_a, W,
                     stride_w, V, ldv, stride_v, info);
  return hipGetLastError();
}

}  // namespace spx_eigh

// ------------------------------------------------------------------ C ABI
extern "C" int spx_syevj_plan(int dtype, int64_t* nmax, int64_t* sweep_max) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_syevj_plan: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_syevj_plan: dtype %d is not float32 / float64", dtype);
  if (nmax) *nmax = spx_eigh::nmax_of(dtype == SPX_F32 ? 4 : 8);
  if (sweep_max) *sweep_max = spx_eigh::SWEEP_MAX;
  return SPX_OK;
}

extern "C" int spx_syevj(int dtype, int uplo, int64_t batch, int64_t n, const void* A, int64_t lda, int64_t stride_a,
                         void* W, int64_t stride_w, void* V, int64_t ldv, int64_t stride_v, int32_t* info,
                         void* stream) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_syevj: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_syevj: dtype %d is not float32 / float64", dtype);
  if (uplo != 0 && uplo != 1) return set_err(SPX_EINVAL, "spx_syevj: uplo %d is not 0 ('L') or 1 ('U')", uplo);
  if (batch < 0 || n < 0)
    return set_err(SPX_EINVAL, "spx_syevj: negative size (batch %lld, n %lld)", (long long)batch, (long long)n);
  const int es = dtype == SPX_F32 ? 4 : 8;
  if (n > spx_eigh::nmax_of(es))
    return set_err(SPX_ENOTSUP, "spx_syevj: n = %lld is above the limit %lld", (long long)n,
                   (long long)spx_eigh::nmax_of(es));
  if (batch > 0x7fffffffLL) return set_err(SPX_ENOTSUP, "spx_syevj: batch = %lld is above 2^31 - 1", (long long)batch);
  if (batch == 0 || n == 0) return SPX_OK;
  if (!A || !W || !V || !info) return set_err(SPX_EINVAL, "spx_syevj: null pointer");
  if (lda < n || ldv < n)
    return set_err(SPX_EINVAL, "spx_syevj: leading dimension (lda %lld, ldv %lld) below n = %lld", (long long)lda,
                   (long long)ldv, (long long)n);
  if (stride_a < 0) return set_err(SPX_EINVAL, "spx_syevj: negative stride_a %lld", (long long)stride_a);
  if (batch > 1 && (stride_w < n || stride_v < (n - 1) * ldv + n))
    return set_err(SPX_EINVAL, "spx_syevj: output strides (stride_w %lld, stride_v %lld) let matrices overlap",
                   (long long)stride_w, (long long)stride_v);
  hipError_t e =
      dtype == SPX_F32
          ? spx_eigh::run<float>(uplo, batch, n, (const float*)A, lda, stride_a, (float*)W, stride_w, (float*)V, ldv,
                                 stride_v, info, S(stream))
          : spx_eigh::run<double>(uplo, batch, n, (const double*)A, lda, stride_a, (double*)W, stride_w, (double*)V,
                                  ldv, stride_v, info, S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_syevj failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

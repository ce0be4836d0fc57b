// Householder TSQR: spx_geqr_plan / spx_geqr_workspace / spx_geqr / spx_orgqr
// (DESIGN.md 3.19).  Included from spx.hip after linalg_kernels.h.
//
// The reduced QR of a tall m x n matrix (m >= n, n <= nmax) as a tree of
// independent block factorizations (communication-avoiding QR, Demmel et al.):
//
//   level 0     ceil(m / r) blocks of up to r rows of A (the rows dealt evenly,
//               so every block has at least n), each factored by ONE
//               workgroup with n Householder reflectors; every block leaves its
//               n x n upper-triangular R in a stack (blocks * n rows);
//   level l+1   the same kernel over level l's stack;
//   ...         until one block remains: its R is the matrix's R.
//
// r = r(dtype, n) >= 2 n, so every level at least halves the stack.  A is read
// once; every block's reflectors (n columns of r numbers, the unit head and the
// zeros above it stored explicitly) and taus stay in the workspace, which is all
// spx_orgqr needs: it walks the tree downwards, block b of a level seeded with
// rows b n .. (b+1) n of the level above's result, applying the block's
// reflectors in reverse order to [seed; 0].
//
// One block in LDS: column k of the block at a[k * RS + i], RS = r + 1 (an odd
// number of 4-byte words for float, of 8-byte words for double: the lanes of a
// wave walk a column at unit stride and the transposing load / store walk a row
// at stride RS, both without a bank conflict), rows past the block's own zero.
// The workgroup is NW waves; lane l of every wave owns rows l, l + 64, ... .
// Factoring column j, EVERY wave reads column j into registers and derives the
// same beta, tau and v from it (the same operations on the same data: the same
// bits), so nothing is broadcast; wave w then updates columns j + 1 + w,
// j + 1 + w + NW, ... (a dot product reduced by __shfl_xor, then one FMA per
// element) and the waves meet at one barrier per column.  Forming Q, the
// columns are independent: wave w owns columns w, w + NW, ... for the whole
// backward sweep and no barrier is needed between reflectors.
//
// Column norms: float data accumulates its squares in double (no float square
// leaves double's range); double data is scaled by the power of two of its
// largest magnitude first (exact), so a representable norm neither overflows
// nor underflows to zero.  A zero column below the diagonal gives tau = 0
// (H = I): no division, no NaN.  No atomics, no inter-workgroup waiting.
//
// The top block alone normalises signs: D = diag(sign(R_jj)) is stored beside
// the reflectors, R's rows are scaled by it and spx_orgqr scales its top seed's
// rows by it, so diag(R) >= 0 and Q R is unchanged (D D = I).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace spx_qr {

typedef int64_t i64;

constexpr int NW = 8;                        // waves per workgroup
constexpr int THREADS = NW * 64;
constexpr int MAX_RPL = 16;                  // rows per lane: r <= 1024
constexpr i64 LDS_BYTES = 160 * 1024;        // what one workgroup may declare
constexpr int MAX_LEVELS = 48;               // blocks at least halve per level

__host__ __device__ inline i64 nmax_of(int esize) { return esize == 4 ? 128 : 64; }

// Rows per block: the largest multiple of 64 (at most 64 MAX_RPL) whose block
// (n columns of r + 1) and diagonal (n) fit the LDS.  >= 2 n for n <= nmax.
inline i64 rows_of(int esize, i64 n) {
  const i64 elems = LDS_BYTES / esize;
  i64 rpl = ((elems - n) / n - 1) / 64;
  if (rpl > MAX_RPL) rpl = MAX_RPL;
  return rpl * 64;
}

inline size_t lds_bytes(int esize, i64 n, i64 r) { return (size_t)((r + 1) * n + n) * esize; }

// ---------------------------------------------------------------- the layout
// The one statement of where everything lives (offsets in elements of the
// data's dtype).  Level l: rows_l rows in nb_l blocks; V (nb r n: block b,
// column j at V + (b n + j) r), tau (nb n) and, below the top, the stack
// (nb n x n, row-major, ld n): level l's Rs = level l + 1's input, and during
// spx_orgqr level l + 1's result (the seeds of level l).  D (n) follows.
struct Level {
  i64 rows, nb, off_v, off_tau, off_stack;
};
struct Layout {
  int levels;
  i64 r, total;  // total elements
  i64 off_d;
  Level lv[MAX_LEVELS];
};

inline bool layout(int esize, i64 m, i64 n, Layout* L) {
  const i64 r = rows_of(esize, n);
  L->r = r;
  L->levels = 0;
  i64 off = 0, rows = m;
  for (;;) {
    if (L->levels == MAX_LEVELS) return false;
    Level& v = L->lv[L->levels++];
    v.rows = rows;
    v.nb = (rows + r - 1) / r;
    v.off_v = off;
    off += v.nb * r * n;
    v.off_tau = off;
    off += v.nb * n;
    v.off_stack = off;
    if (v.nb == 1) break;
    off += v.nb * n * n;
    rows = v.nb * n;
  }
  L->off_d = off;
  L->total = off + n;
  return true;
}

// The rows of a level are dealt to its nb = ceil(rows / r) blocks evenly: block
// b starts at this row.  With rows >= n every block then has at least n rows
// (nb >= 2 means rows > (nb - 1) r, so rows / nb > r / 2 >= n): no block's Q
// has to be cut below its n x n seed, which only a full-rank R would allow.
__host__ __device__ inline i64 block_row(i64 rows, i64 nb, i64 b) {
  const i64 q = rows / nb, rem = rows % nb;
  return b * q + (b < rem ? b : rem);
}

// ------------------------------------------------------------------ kernels
template <typename T>
__device__ inline T wave_sum(T x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

template <typename T>
__device__ inline T wave_max(T x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T y = __shfl_xor(x, o, 64);
    x = y > x ? y : x;
  }
  return x;
}

__device__ inline float fma_t(float a, float b, float c) { return fmaf(a, b, c); }
__device__ inline double fma_t(double a, double b, double c) { return fma(a, b, c); }

// beta, tau and (in x) v of the reflector of the column whose rows >= j this
// wave holds in x (rows < j: 0); alpha = the element of row j.
template <typename T, int RPL>
__device__ inline void reflector(T (&x)[RPL], int j, int lane, T alpha, T& beta, T& tau) {
  T nrm;
  bool zero;
  if constexpr (sizeof(T) == 4) {
    double ss = 0.0;
#pragma unroll
    for (int q = 0; q < RPL; ++q)
      if (q * 64 + lane > j) ss += (double)x[q] * (double)x[q];
    ss = wave_sum(ss);
    zero = ss == 0.0;
    nrm = (T)sqrt(ss + (double)alpha * (double)alpha);
  } else {
    T big = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q)
      if (q * 64 + lane > j) big = fmax(big, fabs(x[q]));
    big = wave_max(big);
    zero = big == 0;
    big = fmax(big, fabs(alpha));
    const int e = zero ? 0 : ilogb(big);
    T ss = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q)
      if (q * 64 + lane > j) {
        const T s = ldexp(x[q], -e);
        ss += s * s;
      }
    ss = wave_sum(ss);
    const T as = ldexp(alpha, -e);
    nrm = ldexp(sqrt(ss + as * as), e);
  }
  if (zero) {
    beta = alpha;
    tau = 0;
    return;
  }
  beta = alpha >= 0 ? -nrm : nrm;
  tau = (beta - alpha) / beta;
  const T d = alpha - beta;
#pragma unroll
  for (int q = 0; q < RPL; ++q) {
    const int i = q * 64 + lane;
    x[q] = i > j ? x[q] / d : (i == j ? (T)1 : (T)0);
  }
}

// Apply H = I - tau v v^T (v in x, zero above row j) to CN columns of the block
// at once: columns k0, k0 + ks, ...; their CN dot products are reduced side by
// side so that the shuffles of one hide behind the others'.  Per column the
// operations, and so the bits, are the same for every CN.
template <typename T, int RPL, int CN>
__device__ inline void apply_reflector(const T (&x)[RPL], T tau, T* a, int RS, int k0, int ks, int j, int lane) {
  T dot[CN];
#pragma unroll
  for (int c = 0; c < CN; ++c) dot[c] = 0;
#pragma unroll
  for (int q = 0; q < RPL; ++q)
    if (q * 64 + 63 >= j) {
#pragma unroll
      for (int c = 0; c < CN; ++c) dot[c] = fma_t(x[q], a[(k0 + c * ks) * RS + q * 64 + lane], dot[c]);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < CN; ++c) dot[c] += __shfl_xor(dot[c], o, 64);
  }
#pragma unroll
  for (int c = 0; c < CN; ++c) dot[c] = -tau * dot[c];
#pragma unroll
  for (int q = 0; q < RPL; ++q)
    if (q * 64 + 63 >= j) {
#pragma unroll
      for (int c = 0; c < CN; ++c) {
        T* p = a + (k0 + c * ks) * RS + q * 64 + lane;
        *p = fma_t(dot[c], x[q], *p);
      }
    }
}

template <typename T, int RPL>
__device__ inline void apply_reflector_from(const T (&x)[RPL], T tau, T* a, int RS, int k, int n, int j, int lane) {
  for (; k + 3 * NW < n; k += 4 * NW) apply_reflector<T, RPL, 4>(x, tau, a, RS, k, NW, j, lane);
  for (; k + NW < n; k += 2 * NW) apply_reflector<T, RPL, 2>(x, tau, a, RS, k, NW, j, lane);
  for (; k < n; k += NW) apply_reflector<T, RPL, 1>(x, tau, a, RS, k, NW, j, lane);
}

// One workgroup factors block b's rows of the `rows` x n matrix A (ld lda); writes
// its reflectors, taus and its n x n R (rows b n .. of Rout, ld ldr; with
// `dsign` the rows scaled to a non-negative diagonal and the signs stored).
template <typename T, int RPL>
__global__ __launch_bounds__(THREADS) void k_geqr_block(const T* __restrict__ A, i64 lda, i64 rows, int n,
                                                        T* __restrict__ V, T* __restrict__ tau_out,
                                                        T* __restrict__ Rout, i64 ldr, T* __restrict__ dsign) {
  extern __shared__ __attribute__((aligned(16))) unsigned char qr_smem[];
  constexpr int R = RPL * 64, RS = R + 1;
  T* a = (T*)qr_smem;
  T* diag = a + (i64)n * RS;
  const i64 b = blockIdx.x;
  const i64 row0 = block_row(rows, gridDim.x, b);
  const int mine = (int)(block_row(rows, gridDim.x, b + 1) - row0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int idx = tid; idx < R * n; idx += THREADS) {
    const int i = idx / n, k = idx - i * n;
    a[k * RS + i] = i < mine ? A[(row0 + i) * lda + k] : (T)0;
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    T x[RPL];
    const T* cj = a + j * RS;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
      const int i = q * 64 + lane;
      x[q] = (q * 64 + 63 >= j && i >= j) ? cj[i] : (T)0;
    }
    const T alpha = cj[j];
    T beta, tau;
    reflector<T, RPL>(x, j, lane, alpha, beta, tau);
    if (wave == j % NW) {
      T* vj = V + (b * n + j) * R;
      if (tau == 0) {
#pragma unroll
        for (int q = 0; q < RPL; ++q) vj[q * 64 + lane] = (q * 64 + lane == j) ? (T)1 : (T)0;
      } else {
#pragma unroll
        for (int q = 0; q < RPL; ++q) vj[q * 64 + lane] = x[q];
      }
      if (lane == 0) {
        tau_out[b * n + j] = tau;
        diag[j] = beta;
      }
    }
    if (tau != 0) apply_reflector_from<T, RPL>(x, tau, a, RS, j + 1 + wave, n, j, lane);
    __syncthreads();
  }
  for (int idx = tid; idx < n * n; idx += THREADS) {
    const int j = idx / n, k = idx - j * n;
    const T d = diag[j];
    T v = k > j ? a[k * RS + j] : (k == j ? d : (T)0);
    if (dsign != nullptr) {
      const T s = d < 0 ? (T)-1 : (T)1;
      if (k >= j) v *= s;
      if (k == j) dsign[j] = s;
    }
    Rout[(b * n + j) * ldr + k] = v;
  }
}

// One workgroup forms block b's rows of the level's result (`rows` x n, ld ldo):
// H_0 ... H_{n-1} [S_b; 0], S_b = rows b n .. of `seed` (ld lds; null: the
// identity), its rows scaled by dsign where given (the top block).
template <typename T, int RPL>
__global__ __launch_bounds__(THREADS) void k_orgqr_block(const T* __restrict__ V, const T* __restrict__ tau_in,
                                                         const T* __restrict__ seed, i64 lds,
                                                         const T* __restrict__ dsign, T* __restrict__ out, i64 ldo,
                                                         i64 rows, int n) {
  extern __shared__ __attribute__((aligned(16))) unsigned char qr_smem[];
  constexpr int R = RPL * 64, RS = R + 1;
  T* a = (T*)qr_smem;
  const i64 b = blockIdx.x;
  const i64 row0 = block_row(rows, gridDim.x, b);
  const int mine = (int)(block_row(rows, gridDim.x, b + 1) - row0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int idx = tid; idx < R * n; idx += THREADS) {
    const int i = idx / n, k = idx - i * n;
    T s = 0;
    if (i < n) {
      s = seed != nullptr ? seed[(b * n + i) * lds + k] : (i == k ? (T)1 : (T)0);
      if (dsign != nullptr) s *= dsign[i];
    }
    a[k * RS + i] = s;
  }
  __syncthreads();
  for (int j = n - 1; j >= 0; --j) {
    const T tau = tau_in[b * n + j];
    if (tau == 0) continue;
    const T* vj = V + (b * n + j) * R;
    T x[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) x[q] = (q * 64 + 63 >= j) ? vj[q * 64 + lane] : (T)0;
    apply_reflector_from<T, RPL>(x, tau, a, RS, wave, n, j, lane);
  }
  __syncthreads();
  for (int idx = tid; idx < mine * n; idx += THREADS) {
    const int i = idx / n, k = idx - i * n;
    out[(row0 + i) * ldo + k] = a[k * RS + i];
  }
}

// ---------------------------------------------------------------- launchers
template <typename T, int RPL>
static hipError_t launch_geqr(i64 nb, size_t lds, hipStream_t s, const T* A, i64 lda, i64 rows, int n, T* V, T* tau,
                              T* Rout, i64 ldr, T* dsign) {
  hipError_t e = hipFuncSetAttribute((const void*)k_geqr_block<T, RPL>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_geqr_block<T, RPL>), dim3((unsigned)nb), dim3(THREADS), lds, s, A, lda, rows, n, V, tau, Rout,
                     ldr, dsign);
  return hipGetLastError();
}

template <typename T, int RPL>
static hipError_t launch_orgqr(i64 nb, size_t lds, hipStream_t s, const T* V, const T* tau, const T* seed, i64 ldseed,
                               const T* dsign, T* out, i64 ldo, i64 rows, int n) {
  hipError_t e = hipFuncSetAttribute((const void*)k_orgqr_block<T, RPL>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_orgqr_block<T, RPL>), dim3((unsigned)nb), dim3(THREADS), lds, s, V, tau, seed, ldseed, dsign,
                     out, ldo, rows, n);
  return hipGetLastError();
}

#define SPX_QR_RPL_CASES(X) \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

template <typename T>
static hipError_t geqr_run(const Layout& L, i64 n, const T* A, i64 lda, T* R, i64 ldr, T* ws, hipStream_t s) {
  const size_t lds = lds_bytes(sizeof(T), n, L.r);
  for (int l = 0; l < L.levels; ++l) {
    const Level& v = L.lv[l];
    const bool top = l == L.levels - 1;
    const T* in = l == 0 ? A : ws + L.lv[l - 1].off_stack;
    const i64 ldin = l == 0 ? lda : n;
    T* out = top ? R : ws + v.off_stack;
    const i64 ldout = top ? ldr : n;
    T* d = top ? ws + L.off_d : nullptr;
    hipError_t e = hipErrorInvalidValue;
    switch (L.r / 64) {
#define X(P)                                                                                               \
  case P:                                                                                                  \
    e = launch_geqr<T, P>(v.nb, lds, s, in, ldin, v.rows, (int)n, ws + v.off_v, ws + v.off_tau, out, ldout, d); \
    break;
      SPX_QR_RPL_CASES(X)
#undef X
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename T>
static hipError_t orgqr_run(const Layout& L, i64 n, T* ws, const T* C, i64 ldc, T* Q, i64 ldq, hipStream_t s) {
  const size_t lds = lds_bytes(sizeof(T), n, L.r);
  for (int l = L.levels - 1; l >= 0; --l) {
    const Level& v = L.lv[l];
    const bool top = l == L.levels - 1;
    const T* seed = top ? C : ws + v.off_stack;  // the level above's result lies in this level's stack
    const i64 ldseed = top ? ldc : n;
    const T* d = top ? ws + L.off_d : nullptr;
    T* out = l == 0 ? Q : ws + L.lv[l - 1].off_stack;
    const i64 ldout = l == 0 ? ldq : n;
    hipError_t e = hipErrorInvalidValue;
    switch (L.r / 64) {
#define X(P)                                                                                                  \
  case P:                                                                                                     \
    e = launch_orgqr<T, P>(v.nb, lds, s, ws + v.off_v, ws + v.off_tau, seed, ldseed, d, out, ldout, v.rows, (int)n); \
    break;
      SPX_QR_RPL_CASES(X)
#undef X
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace spx_qr

// ------------------------------------------------------------------ C ABI
static const int64_t QR_ROWS_MAX = (1LL << 38);  // r >= 256: below 2^30 blocks a level

extern "C" int spx_geqr_plan(int dtype, int64_t n, int64_t* nmax, int64_t* rows) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_geqr_plan: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_geqr_plan: dtype %d is not float32 / float64", dtype);
  if (n < 0) return set_err(SPX_EINVAL, "spx_geqr_plan: negative n = %lld", (long long)n);
  const int es = dtype == SPX_F32 ? 4 : 8;
  const int64_t lim = spx_qr::nmax_of(es);
  if (nmax) *nmax = lim;
  if (rows) *rows = n > lim ? 0 : spx_qr::rows_of(es, n < 1 ? 1 : n);
  return SPX_OK;
}

extern "C" int64_t spx_geqr_workspace(int dtype, int64_t m, int64_t n) {
  const int es = dtype == SPX_F32 ? 4 : 8;
  spx_qr::Layout L;
  if (!linalg_dtype(dtype) || m < 0 || n < 0 || m < n || m > QR_ROWS_MAX || n > spx_qr::nmax_of(es)) {
    set_err(SPX_EINVAL, "spx_geqr_workspace: bad arguments (dtype %d, m %lld, n %lld)", dtype, (long long)m,
            (long long)n);
    return -1;
  }
  if (m == 0 || n == 0) return 0;
  if (!spx_qr::layout(es, m, n, &L)) {
    set_err(SPX_EINVAL, "spx_geqr_workspace: too many levels for m %lld, n %lld", (long long)m, (long long)n);
    return -1;
  }
  return L.total * es;
}

static int qr_check(const char* who, int dtype, int64_t m, int64_t n, spx_qr::Layout* L) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "%s: bad dtype %d", who, dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "%s: dtype %d is not float32 / float64", who, dtype);
  if (m < 0 || n < 0) return set_err(SPX_EINVAL, "%s: negative size (%lld, %lld)", who, (long long)m, (long long)n);
  if (m < n) return set_err(SPX_EINVAL, "%s: m = %lld < n = %lld (a tall or square matrix is needed)", who,
                            (long long)m, (long long)n);
  const int es = dtype == SPX_F32 ? 4 : 8;
  if (n > spx_qr::nmax_of(es))
    return set_err(SPX_ENOTSUP, "%s: n = %lld is above the column limit %lld", who, (long long)n,
                   (long long)spx_qr::nmax_of(es));
  if (m > QR_ROWS_MAX) return set_err(SPX_ENOTSUP, "%s: m = %lld is above 2^38", who, (long long)m);
  if (m > 0 && n > 0 && !spx_qr::layout(es, m, n, L)) return set_err(SPX_ENOTSUP, "%s: too many levels", who);
  return SPX_OK;
}

extern "C" int spx_geqr(int dtype, int64_t m, int64_t n, const void* A, int64_t lda, void* R, int64_t ldr,
                        void* workspace, size_t workspace_bytes, void* stream) {
  spx_qr::Layout L;
  int rc = qr_check("spx_geqr", dtype, m, n, &L);
  if (rc != SPX_OK) return rc;
  if (m > 0 && n > 0 && (!A || !R)) return set_err(SPX_EINVAL, "spx_geqr: null matrix");
  if (lda < n || ldr < n)
    return set_err(SPX_EINVAL, "spx_geqr: leading dimension (lda %lld, ldr %lld) below n = %lld", (long long)lda,
                   (long long)ldr, (long long)n);
  if (m == 0 || n == 0) return SPX_OK;
  const int es = dtype == SPX_F32 ? 4 : 8;
  if (!workspace || (int64_t)workspace_bytes < L.total * es)
    return set_err(SPX_EINVAL, "spx_geqr: workspace too small (%lld bytes needed)", (long long)(L.total * es));
  hipError_t e = dtype == SPX_F32 ? spx_qr::geqr_run<float>(L, n, (const float*)A, lda, (float*)R, ldr,
                                                            (float*)workspace, S(stream))
                                  : spx_qr::geqr_run<double>(L, n, (const double*)A, lda, (double*)R, ldr,
                                                             (double*)workspace, S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_geqr failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

extern "C" int spx_orgqr(int dtype, int64_t m, int64_t n, void* workspace, size_t workspace_bytes, const void* C,
                         int64_t ldc, void* Q, int64_t ldq, void* stream) {
  spx_qr::Layout L;
  int rc = qr_check("spx_orgqr", dtype, m, n, &L);
  if (rc != SPX_OK) return rc;
  if (m > 0 && n > 0 && !Q) return set_err(SPX_EINVAL, "spx_orgqr: null matrix");
  if (ldq < n || (C && ldc < n))
    return set_err(SPX_EINVAL, "spx_orgqr: leading dimension (ldc %lld, ldq %lld) below n = %lld", (long long)ldc,
                   (long long)ldq, (long long)n);
  if (m == 0 || n == 0) return SPX_OK;
  const int es = dtype == SPX_F32 ? 4 : 8;
  if (!workspace || (int64_t)workspace_bytes < L.total * es)
    return set_err(SPX_EINVAL, "spx_orgqr: workspace too small (%lld bytes needed)", (long long)(L.total * es));
  hipError_t e = dtype == SPX_F32 ? spx_qr::orgqr_run<float>(L, n, (float*)workspace, (const float*)C, ldc, (float*)Q,
                                                             ldq, S(stream))
                                  : spx_qr::orgqr_run<double>(L, n, (double*)workspace, (const double*)C, ldc,
                                                              (double*)Q, ldq, S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_orgqr failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

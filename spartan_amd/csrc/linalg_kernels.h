// Dense Cholesky for gfx950: spx_potrf, spx_trsm and spx_syrk,
// included by spx.hip after gemm_kernels.h (Mfma<T>).  Replaces the three
// LAPACK / BLAS mappers of spartan/examples/cholesky.py (_cholesky_dpotrf_mapper,
// _cholesky_dtrsm_mapper, _cholesky_dsyrk_dgemm_mapper).
//
// Everything is row-major with leading dimensions in elements and runs in
// place on the lower triangle.
//
//   k_update      C[M,N] -= A[M,K] op(B): the NT product (B[N,K], read along
//                 its rows) or, for the trsm RIGHT/N sweep only, the NN product
//                 (B[K,N]).  A 128 x BN block tile (BN 128 or 64), 2 x 2 waves,
//                 K-tiles of 128 bytes; both operands are staged k-contiguous in
//                 LDS (rows padded by one element), the next K-tile's global
//                 loads are in flight during the MFMAs.  One accumulation chain
//                 per element; C is read and written once, in the epilogue.
//                 LOWER: the grid is the lower triangle of the tile grid (block
//                 b -> (tm, tn), tn <= tm) and diagonal tiles touch only i >= j.
//   k_potrf_diag  one workgroup factors a diagonal block of up to NB = 64 held
//                 in registers (right-looking, the column published through
//                 LDS and scaled by a true division, the pivot's square root
//                 correctly rounded).  A block shorter than NB is padded with
//                 the identity, so every loop has a fixed trip count; the first
//                 non-positive or NaN pivot is remembered by one thread and
//                 written to *info if *info is still 0.
//   k_trsm_diag   X op(L_jj) = B for one diagonal block: a quad of lanes keeps
//                 a row of B in registers and substitutes with true divisions,
//                 the quotient broadcast inside the quad; L_jj is read from
//                 LDS.  op = N is the same ascending sweep on the block
//                 reversed in both indices, so there is one substitution loop.
//   k_tril_copy   L = tril(A), strict upper triangle +0.0 (A's is never read).
//   k_transpose   B -> B^T through a 32 x 32 LDS tile (the LEFT forms of trsm).
//
// potrf is blocked at two levels: panels of NBO = 512 columns are factored by
// the one-level algorithm on NB = 64 (diag, panel solve, lower update within
// the panel's diagonal block), the rows below are solved by the blocked trsm
// RIGHT/T, and the trailing matrix takes one lower update with K = NBO -- an
// eighth of the C traffic of eight K = NB updates.  trsm RIGHT is
// right-looking: each solved block of NB columns is at once subtracted from
// the columns still to solve (K = NB updates over many tiles), so a few rows
// of B still fill the GPU.  LEFT forms run the RIGHT kernels on a transposed
// copy of B in the workspace.
//
// No kernel waits for another workgroup, none uses atomics, no loop bound
// depends on data: after a failed pivot everything still runs to the end.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace spx_linalg {

using spx_mfma::Mfma;
typedef int64_t i64;

constexpr int NB = 64;    // diagonal block: one workgroup, LDS
constexpr int NBO = 512;  // outer panel: K of the trailing update
constexpr int UBM = 128;  // update kernel's block rows

// ------------------------------------------------------------------ update
template <typename T, int BN, bool NN, bool LOWER>
__global__ __launch_bounds__(256) void k_update(i64 M, i64 N, i64 K, const T* A, i64 lda, const T* B, i64 ldb, T* C,
                                                i64 ldc, int tiles_n) {
  typedef Mfma<T> F;
  constexpr int BM = UBM;
  constexpr int BK = 128 / sizeof(T);
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = WTM / F::TILE, TN = WTN / F::TILE;
  constexpr int LA = BM * BK / 256, LB = BN * BK / 256;
  static_assert(TM >= 1 && TN >= 1 && BK % F::KS == 0 && (!LOWER || BM == BN), "bad tiling");
  __shared__ T As[BM][BK + 1];
  __shared__ T Bs[BN][BK + 1];
  int tm, tn;
  if constexpr (LOWER) {  // block b of the lower triangle, row by row
    const i64 b = blockIdx.x;
    i64 r = (i64)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > b) --r;
    while ((r + 1) * (r + 2) / 2 <= b) ++r;
    tm = (int)r;
    tn = (int)(b - r * (r + 1) / 2);
  } else {
    tm = blockIdx.x / tiles_n;
    tn = blockIdx.x - tm * tiles_n;
  }
  const i64 row0 = (i64)tm * BM, col0 = (i64)tn * BN;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wm = w >> 1, wn = w & 1;
  typename F::acc_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = F::zero();
  T ra[LA], rb[LB];
  auto load = [&](i64 k0) {
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int idx = t + i * 256;
      const i64 gr = row0 + idx / BK, gk = k0 + idx % BK;
      ra[i] = (gr < M && gk < K) ? A[gr * lda + gk] : (T)0;
    }
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      const int idx = t + i * 256;
      if constexpr (NN) {
        const i64 gk = k0 + idx / BN, gc = col0 + idx % BN;
        rb[i] = (gk < K && gc < N) ? B[gk * ldb + gc] : (T)0;
      } else {
        const i64 gc = col0 + idx / BK, gk = k0 + idx % BK;
        rb[i] = (gc < N && gk < K) ? B[gc * ldb + gk] : (T)0;
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int idx = t + i * 256;
      As[idx / BK][idx % BK] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      const int idx = t + i * 256;
      if constexpr (NN)
        Bs[idx % BN][idx / BN] = rb[i];
      else
        Bs[idx / BK][idx % BK] = rb[i];
    }
  };
  const int nk = (int)((K + BK - 1) / BK);
  load(0);
  for (int kt = 0; kt < nk; ++kt) {
    store();
    __syncthreads();
    if (kt + 1 < nk) load((i64)(kt + 1) * BK);
#pragma unroll
    for (int kk = 0; kk < BK / F::KS; ++kk) {
      const int k = kk * F::KS + F::opk(lane);
      T a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = As[wm * WTM + i * F::TILE + F::opi(lane)][k];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = Bs[wn * WTN + j * F::TILE + F::opi(lane)][k];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = F::mma(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < F::NREG; ++r) {
        const i64 gr = row0 + wm * WTM + i * F::TILE + F::crow(lane, r);
        const i64 gc = col0 + wn * WTN + j * F::TILE + F::ccol(lane);
        if (gr < M && gc < N && (!LOWER || gc <= gr)) C[gr * ldc + gc] = C[gr * ldc + gc] - acc[i][j][r];
      }
}

// number of update blocks, or -1 where it does not fit the grid
static inline i64 update_blocks(bool lower, i64 M, i64 N) {
  const i64 tmn = (M + UBM - 1) / UBM;
  const i64 bn = (!lower && N <= 64) ? 64 : 128;
  const i64 tnn = (N + bn - 1) / bn;
  if (tmn >= (1LL << 24) || tnn >= (1LL << 24)) return -1;
  const i64 nt = lower ? tmn * (tmn + 1) / 2 : tmn * tnn;
  return nt < (1LL << 31) ? nt : -1;
}

template <typename T>
static hipError_t update(bool nn, bool lower, i64 M, i64 N, i64 K, const T* A, i64 lda, const T* B, i64 ldb, T* C,
                         i64 ldc, hipStream_t s) {
  if (M <= 0 || N <= 0 || K <= 0) return hipSuccess;
  const unsigned nt = (unsigned)update_blocks(lower, M, N);
  if (lower) {
    k_update<T, 128, false, true><<<nt, 256, 0, s>>>(M, N, K, A, lda, B, ldb, C, ldc, 0);
  } else if (N <= 64) {
    if (nn)
      k_update<T, 64, true, false><<<nt, 256, 0, s>>>(M, N, K, A, lda, B, ldb, C, ldc, 1);
    else
      k_update<T, 64, false, false><<<nt, 256, 0, s>>>(M, N, K, A, lda, B, ldb, C, ldc, 1);
  } else {
    const int tnn = (int)((N + 127) / 128);
    if (nn)
      k_update<T, 128, true, false><<<nt, 256, 0, s>>>(M, N, K, A, lda, B, ldb, C, ldc, tnn);
    else
      k_update<T, 128, false, false><<<nt, 256, 0, s>>>(M, N, K, A, lda, B, ldb, C, ldc, tnn);
  }
  return hipGetLastError();
}

// ------------------------------------------------------- diagonal block potrf
template <typename T>
__device__ __forceinline__ T sqrt_rn(T x);
template <>
__device__ __forceinline__ float sqrt_rn<float>(float x) {
  return sqrtf(x);
}
template <>
__device__ __forceinline__ double sqrt_rn<double>(double x) {
  return sqrt(x);
}

// L (jn x jn, jn <= NB, row stride ld) is factored in place; `base` is the
// block's first row in the whole matrix.  The block lives in registers: thread
// (ty, tx) = (t / 16, t % 16) holds the 4 x 4 elements (ty + 16 a, tx + 16 b).
// Step j: the owners of column j publish it; wave 0 takes the square root of
// the pivot and divides one element of the column each; every thread subtracts
// the column's outer product from its elements right of j.  The j loop is
// unrolled, so the owners' register index is a constant.
template <typename T>
__global__ __launch_bounds__(256) void k_potrf_diag(T* L, i64 ld, int jn, int base, int* info) {
  __shared__ T craw[NB], scol[NB];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  T v[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = ty + 16 * a, j = tx + 16 * b;
      v[a][b] = (i < jn && j <= i) ? L[(i64)i * ld + j] : ((i == j) ? (T)1 : (T)0);
    }
  int fail = 0;  // thread 0's
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int bj = j >> 4;
    if (tx == (j & 15)) {
#pragma unroll
      for (int a = 0; a < 4; ++a) craw[ty + 16 * a] = v[a][bj];
    }
    __syncthreads();
    if (t < NB) {
      const T d = craw[j];
      if (t == 0 && !(d > (T)0) && fail == 0) fail = j + 1;
      const T l = sqrt_rn<T>(d);
      scol[t] = (t == j) ? l : (t > j ? craw[t] / l : (T)0);
    }
    __syncthreads();
    T li[4], lj[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) li[a] = scol[ty + 16 * a];
#pragma unroll
    for (int b = 0; b < 4; ++b) lj[b] = scol[tx + 16 * b];
    if (tx == (j & 15)) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
        if (ty + 16 * a >= j) v[a][bj] = li[a];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (ty + 16 * a > j && tx + 16 * b > j) v[a][b] = v[a][b] - li[a] * lj[b];
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = ty + 16 * a, j = tx + 16 * b;
      if (i < jn && j <= i) L[(i64)i * ld + j] = v[a][b];
    }
  if (t == 0 && fail != 0 && fail <= jn && *info == 0) *info = base + fail;
}

// ---------------------------------------------------- diagonal block solve
// TRANS: X L^T = B, else X L = B, for the jn x jn block L (jn <= NB) and the
// M x jn block B, in place; 64 rows of B per workgroup.  A row of B is
// independent of the others, so it stays inside one quad of lanes: lane q of
// the quad holds the row's columns 16 q .. 16 q + 15 in registers, in sweep
// order (ascending for TRANS; for op = N the block is reversed in both
// indices, so the sweep is the same ascending one).  Step j: the lane that
// holds column j divides by the diagonal (a true division), the quotient is
// broadcast inside the quad, and each lane subtracts x_j L[s][j] from its
// columns s > j.  L is read from LDS as Lt[j][s], so a lane's 16 coefficients
// are 16-byte reads; no barrier inside the sweep.
template <typename T, bool TRANS>
__global__ __launch_bounds__(256) void k_trsm_diag(const T* L, i64 ldl, int jn, T* B, i64 ldb, i64 M) {
  constexpr int VE = 16 / sizeof(T), LS = NB + VE;
  typedef T V __attribute__((ext_vector_type(VE)));
  // Lt[k][s]: the coefficient of x_k in equation s (sweep order), lower, padded with the identity
  __shared__ __attribute__((aligned(16))) T Lt[NB][LS];
  const int t = threadIdx.x, q = t & 3, lane = t & 63;
  const i64 row = (i64)blockIdx.x * 64 + (t >> 2);
  for (int idx = t; idx < NB * NB; idx += 256) {
    const int r = idx / NB, c = idx % NB;
    T x = (r == c) ? (T)1 : (T)0;
    if (r < jn && c <= r) x = L[(i64)r * ldl + c];
    if (TRANS)
      Lt[c][r] = x;
    else
      Lt[NB - 1 - r][NB - 1 - c] = x;
  }
  T v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int s = 16 * q + i, c = TRANS ? s : NB - 1 - s;
    v[i] = (row < M && c < jn) ? B[row * ldb + c] : (T)0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int bj = j >> 4, ij = j & 15;
    T lrow[16];
#pragma unroll
    for (int i = 0; i < 16; i += VE) {
      const V w = *(const V*)&Lt[j][16 * q + i];
#pragma unroll
      for (int e = 0; e < VE; ++e) lrow[i + e] = w[e];
    }
    T xj = v[ij] / Lt[j][j];                  // every lane divides; the quotient of the lane holding column j counts
    xj = __shfl(xj, (lane & ~3) | bj);
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (16 * q + i > j) v[i] = v[i] - xj * lrow[i];
    if (q == bj) v[ij] = xj;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int s = 16 * q + i, c = TRANS ? s : NB - 1 - s;
    if (row < M && c < jn) B[row * ldb + c] = v[i];
  }
}

template <typename T, bool TRANS>
static hipError_t trsm_diag(const T* L, i64 ldl, int jn, T* B, i64 ldb, i64 M, hipStream_t s) {
  if (M <= 0 || jn <= 0) return hipSuccess;
  k_trsm_diag<T, TRANS><<<(unsigned)((M + 63) / 64), 256, 0, s>>>(L, ldl, jn, B, ldb, M);
  return hipGetLastError();
}

// X op(L) = B, L n x n lower, B M x n, in place; right-looking over blocks
template <typename T>
static hipError_t trsm_right(bool trans, i64 M, i64 n, const T* L, i64 ldl, T* B, i64 ldb, hipStream_t s) {
  hipError_t e;
  if (trans) {
    for (i64 j = 0; j < n; j += NB) {
      const int jb = (int)(n - j < NB ? n - j : NB);
      if ((e = trsm_diag<T, true>(L + j * ldl + j, ldl, jb, B + j, ldb, M, s)) != hipSuccess) return e;
      const i64 rest = n - j - jb;  // B[:, j + jb:] -= X[:, j:j + jb] L[j + jb:, j:j + jb]^T
      if ((e = update<T>(false, false, M, rest, jb, B + j, ldb, L + (j + jb) * ldl + j, ldl, B + j + jb, ldb, s)) !=
          hipSuccess)
        return e;
    }
  } else {
    for (i64 j = (n - 1) / NB * NB; j >= 0; j -= NB) {
      const int jb = (int)(n - j < NB ? n - j : NB);
      if ((e = trsm_diag<T, false>(L + j * ldl + j, ldl, jb, B + j, ldb, M, s)) != hipSuccess) return e;
      // B[:, :j] -= X[:, j:j + jb] L[j:j + jb, :j]
      if ((e = update<T>(true, false, M, j, jb, B + j, ldb, L + j * ldl, ldl, B, ldb, s)) != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

// ------------------------------------------------------- copies
template <typename T>
__global__ __launch_bounds__(256) void k_tril_copy(i64 n, const T* A, i64 lda, T* L, i64 ldl) {
  const i64 total = n * n;
  for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
    const i64 i = idx / n, j = idx - i * n;
    if (j > i)
      L[i * ldl + j] = (T)0;
    else if (A != L)
      L[i * ldl + j] = A[i * lda + j];
  }
}

// out[c * ldo + r] = in[r * ldi + c], in rows x cols
template <typename T>
__global__ __launch_bounds__(256) void k_transpose(i64 rows, i64 cols, const T* in, i64 ldi, T* out, i64 ldo,
                                                   int tiles_c) {
  __shared__ T tile[32][33];
  const int tr = blockIdx.x / tiles_c, tc = blockIdx.x - tr * tiles_c;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const i64 r = (i64)tr * 32 + i, c = (i64)tc * 32 + tx;
    if (r < rows && c < cols) tile[i][tx] = in[r * ldi + c];
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const i64 c = (i64)tc * 32 + i, r = (i64)tr * 32 + tx;
    if (r < rows && c < cols) out[c * ldo + r] = tile[tx][i];
  }
}

template <typename T>
static hipError_t transpose(i64 rows, i64 cols, const T* in, i64 ldi, T* out, i64 ldo, hipStream_t s) {
  const i64 trn = (rows + 31) / 32, tcn = (cols + 31) / 32;
  k_transpose<T><<<(unsigned)(trn * tcn), 256, 0, s>>>(rows, cols, in, ldi, out, ldo, (int)tcn);
  return hipGetLastError();
}

// -------------------------------------------------------------- potrf driver
template <typename T>
static hipError_t potrf_run(i64 n, const T* A, i64 lda, T* L, i64 ld, int* info, hipStream_t s) {
  hipError_t e;
  if ((e = hipMemsetAsync(info, 0, sizeof(int), s)) != hipSuccess) return e;
  {
    i64 g = (n * n + 255) / 256;
    if (g > 65536) g = 65536;
    k_tril_copy<T><<<(unsigned)g, 256, 0, s>>>(n, A, lda, L, ld);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  for (i64 K0 = 0; K0 < n; K0 += NBO) {
    const i64 KB = n - K0 < NBO ? n - K0 : NBO;
    T* const D = L + K0 * ld + K0;
    for (i64 k = 0; k < KB; k += NB) {  // the panel's diagonal block, one level
      const int kb = (int)(KB - k < NB ? KB - k : NB);
      T* const d = D + k * ld + k;
      k_potrf_diag<T><<<1, 256, 0, s>>>(d, ld, kb, (int)(K0 + k), info);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      const i64 rows = KB - k - kb;
      if (rows > 0) {
        T* const P = d + (i64)kb * ld;
        if ((e = trsm_diag<T, true>(d, ld, kb, P, ld, rows, s)) != hipSuccess) return e;
        if ((e = update<T>(false, true, rows, rows, kb, P, ld, P, ld, P + kb, ld, s)) != hipSuccess) return e;
      }
    }
    const i64 R = n - K0 - KB;
    if (R > 0) {
      T* const P = D + KB * ld;
      if ((e = trsm_right<T>(true, R, KB, D, ld, P, ld, s)) != hipSuccess) return e;
      if ((e = update<T>(false, true, R, R, KB, P, ld, P, ld, P + KB, ld, s)) != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

}  // namespace spx_linalg

// ------------------------------------------------------------------ C ABI
static bool linalg_dtype(int d) { return d == SPX_F32 || d == SPX_F64; }
static const int64_t LINALG_IDX_MAX = (1LL << 31) - 1;

extern "C" int spx_potrf_plan(int dtype, int64_t* nb, int64_t* nb_outer) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_potrf_plan: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_potrf_plan: dtype %d is not float32 / float64", dtype);
  if (nb) *nb = spx_linalg::NB;
  if (nb_outer) *nb_outer = spx_linalg::NBO;
  return SPX_OK;
}

extern "C" int64_t spx_potrf_workspace(int dtype, int64_t n) {
  if (!linalg_dtype(dtype) || n < 0 || n > LINALG_IDX_MAX) {
    set_err(SPX_EINVAL, "spx_potrf_workspace: bad arguments (dtype %d, n %lld)", dtype, (long long)n);
    return -1;
  }
  return 0;  // the factorization runs in place on L
}

extern "C" int spx_potrf(int dtype, int64_t n, const void* A, int64_t lda, void* L, int64_t ldl, int32_t* info,
                         void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace;
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_potrf: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_potrf: dtype %d is not float32 / float64", dtype);
  if (n < 0) return set_err(SPX_EINVAL, "spx_potrf: negative size n = %lld", (long long)n);
  if (!info) return set_err(SPX_EINVAL, "spx_potrf: null info");
  if (n > 0 && (!A || !L)) return set_err(SPX_EINVAL, "spx_potrf: null matrix");
  if (lda < n || ldl < n)
    return set_err(SPX_EINVAL, "spx_potrf: leading dimension (lda %lld, ldl %lld) below n = %lld", (long long)lda,
                   (long long)ldl, (long long)n);
  if (A == L && n > 0 && lda != ldl) return set_err(SPX_EINVAL, "spx_potrf: in place needs lda == ldl");
  if (n > LINALG_IDX_MAX || spx_linalg::update_blocks(true, n, n) < 0)
    return set_err(SPX_ENOTSUP, "spx_potrf: n = %lld reaches 2^31 in the kernels' tile indices", (long long)n);
  const int64_t need = spx_potrf_workspace(dtype, n);
  if ((int64_t)workspace_bytes < need) return set_err(SPX_EINVAL, "spx_potrf: workspace too small");
  if (n == 0) return SPX_OK;
  hipError_t e = dtype == SPX_F32
                     ? spx_linalg::potrf_run<float>(n, (const float*)A, lda, (float*)L, ldl, info, S(stream))
                     : spx_linalg::potrf_run<double>(n, (const double*)A, lda, (double*)L, ldl, info, S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_potrf failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

extern "C" int64_t spx_trsm_workspace(int dtype, int side, int64_t m, int64_t n) {
  if (!linalg_dtype(dtype) || m < 0 || n < 0 || m > LINALG_IDX_MAX || n > LINALG_IDX_MAX ||
      (side != SPX_SIDE_LEFT && side != SPX_SIDE_RIGHT)) {
    set_err(SPX_EINVAL, "spx_trsm_workspace: bad arguments (dtype %d, side %d, m %lld, n %lld)", dtype, side,
            (long long)m, (long long)n);
    return -1;
  }
  if (side == SPX_SIDE_RIGHT) return 0;
  return m * n * (dtype == SPX_F32 ? 4 : 8);  // B transposed
}

extern "C" int spx_trsm(int dtype, int side, int op, int64_t m, int64_t n, const void* L, int64_t ldl, void* B,
                        int64_t ldb, void* workspace, size_t workspace_bytes, void* stream) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_trsm: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_trsm: dtype %d is not float32 / float64", dtype);
  if (side != SPX_SIDE_LEFT && side != SPX_SIDE_RIGHT) return set_err(SPX_EINVAL, "spx_trsm: bad side %d", side);
  if (op != SPX_TRANS_N && op != SPX_TRANS_T) return set_err(SPX_EINVAL, "spx_trsm: bad op %d", op);
  if (m < 0 || n < 0) return set_err(SPX_EINVAL, "spx_trsm: negative size (%lld, %lld)", (long long)m, (long long)n);
  const int64_t nl = side == SPX_SIDE_LEFT ? m : n;
  if (m > 0 && n > 0 && (!L || !B)) return set_err(SPX_EINVAL, "spx_trsm: null matrix");
  if (ldl < nl || ldb < n)
    return set_err(SPX_EINVAL, "spx_trsm: leading dimension (ldl %lld, ldb %lld) too small", (long long)ldl,
                   (long long)ldb);
  if (m > LINALG_IDX_MAX || n > LINALG_IDX_MAX || spx_linalg::update_blocks(false, m, n) < 0 ||
      spx_linalg::update_blocks(false, n, m) < 0 || (m + 31) / 32 * ((n + 31) / 32) > LINALG_IDX_MAX)
    return set_err(SPX_ENOTSUP, "spx_trsm: (%lld, %lld) reaches 2^31 in the kernels' tile indices", (long long)m,
                   (long long)n);
  const int64_t need = spx_trsm_workspace(dtype, side, m, n);
  if ((int64_t)workspace_bytes < need || (need > 0 && !workspace))
    return set_err(SPX_EINVAL, "spx_trsm: workspace too small (%lld bytes needed)", (long long)need);
  if (m == 0 || n == 0) return SPX_OK;
  hipStream_t s = S(stream);
  hipError_t e = hipSuccess;
  auto run = [&](auto zero) -> hipError_t {
    typedef decltype(zero) T;
    const T* l = (const T*)L;
    T* b = (T*)B;
    if (side == SPX_SIDE_RIGHT) return spx_linalg::trsm_right<T>(op == SPX_TRANS_T, m, n, l, ldl, b, ldb, s);
    // op(L) X = B  <=>  X^T op(L)^T = B^T
    T* w = (T*)workspace;
    hipError_t r;
    if ((r = spx_linalg::transpose<T>(m, n, b, ldb, w, m, s)) != hipSuccess) return r;
    if ((r = spx_linalg::trsm_right<T>(op == SPX_TRANS_N, n, m, l, ldl, w, m, s)) != hipSuccess) return r;
    return spx_linalg::transpose<T>(n, m, w, m, b, ldb, s);
  };
  e = dtype == SPX_F32 ? run(0.0f) : run(0.0);
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_trsm failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

extern "C" int spx_syrk(int dtype, int lower, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
                        const void* B, int64_t ldb, void* C, int64_t ldc, void* stream) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_syrk: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_syrk: dtype %d is not float32 / float64", dtype);
  if (M < 0 || N < 0 || K < 0)
    return set_err(SPX_EINVAL, "spx_syrk: negative size (%lld, %lld, %lld)", (long long)M, (long long)N, (long long)K);
  if (lower && M != N) return set_err(SPX_EINVAL, "spx_syrk: lower needs M == N");
  if (M > 0 && N > 0 && (!C || (K > 0 && (!A || !B)))) return set_err(SPX_EINVAL, "spx_syrk: null matrix");
  if (lda < K || ldb < K || ldc < N)
    return set_err(SPX_EINVAL, "spx_syrk: leading dimension (lda %lld, ldb %lld, ldc %lld) too small", (long long)lda,
                   (long long)ldb, (long long)ldc);
  if (M > LINALG_IDX_MAX || N > LINALG_IDX_MAX || K > LINALG_IDX_MAX || spx_linalg::update_blocks(lower != 0, M, N) < 0)
    return set_err(SPX_ENOTSUP, "spx_syrk: (%lld, %lld, %lld) reaches 2^31 in the kernel's tile indices", (long long)M,
                   (long long)N, (long long)K);
  if (M == 0 || N == 0 || K == 0) return SPX_OK;
  hipError_t e =
      dtype == SPX_F32
          ? spx_linalg::update<float>(false, lower != 0, M, N, K, (const float*)A, lda, (const float*)B, ldb, (float*)C,
                                      ldc, S(stream))
          : spx_linalg::update<double>(false, lower != 0, M, N, K, (const double*)A, lda, (const double*)B, ldb,
                                       (double*)C, ldc, S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_syrk failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

// Batched dense SVD: spx_gesvj_plan / spx_gesvj.
// Included from spx.hip after eigh_kernels.h, whose tournament (pair_of), Eps
// and constants it shares.
//
// The reduced SVD A = U diag(S) Vt of `batch` row-major m x n matrices, m >= n,
// by the one-sided (Hestenes) Jacobi method: ONE workgroup per matrix, the grid
// over the batch, nothing but the load and the final store touches global
// memory.  The method works on A itself, never on A^T A, so small singular
// values come out to high relative accuracy.
//
// LDS: the working copy G (m x n) and V (n x n, the identity at the start; not
// there for jobu == 0), both column-major with an odd column stride (m | 1 and
// n | 1): the lanes of a group walk a column at unit stride and the groups of a
// wave start in different banks, the layout argument of qr_kernels.h; the
// finish's singular values and signs, its permutation and one flag word.
//
// Preparation as in k_syevj, from the largest magnitude of A: zero (S = 0,
// Vt = I, U = 0, info = 0), not finite (NaN outputs, info = -1), else G is
// scaled by that magnitude's power of two (exact).
//
// A sweep is the m' - 1 rounds of the round-robin tournament over
// m' = n + (n & 1) column indices.  A group of LP lanes owns a pair (p, q) of the
// round: it forms a_pp = g_p.g_p, a_qq = g_q.g_q, a_pq = g_p.g_q (each lane its
// rows in ascending order, then a butterfly over the group's lanes: every lane
// ends with the same bits), rotates iff a_pp > tiny, a_qq > tiny (tiny = the
// smallest normal number / u: a column below that counts as zero) and
// |a_pq| > tol sqrt(a_pp) sqrt(a_qq), tol = sqrt(m) u (Rutishauser's formulas,
// true divisions), and applies the rotation to columns p, q of G and of V
// itself.  The pairs of a round are disjoint and nobody else touches a group's
// columns, so a round has ONE workgroup barrier, at its end.  The column norms
// are formed anew in every round.  A sweep without a rotation ends the
// iteration; every thread takes that decision from the same LDS word after a
// barrier.  SWEEP_MAX bounds the loop.
//
// Finish: s_j = ||g_j|| (the sum in double, in the same fixed order), its rank
// is the count of the s_i that sort before it (descending, ties by index);
// column j of V becomes row rank of Vt with the sign that makes its entry of
// largest magnitude (the first on a tie) positive, and g_j / s_j with the same
// sign becomes column rank of U -- an exactly zero s_j gives an exactly zero
// column of U (LAPACK gesvj's contract).  S is unscaled by ldexp.
//
// The workgroup size depends on (m, n) alone and no atomics are used: a matrix's
// result is the same bits wherever it stands in a batch.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

namespace spx_svd {

typedef int64_t i64;
using spx_eigh::Eps;
using spx_eigh::LDS_BYTES;
using spx_eigh::MAX_WAVES;
using spx_eigh::pair_of;

constexpr int SWEEP_MAX = 64;

// The one statement of the LDS layout: MAX_WAVES doubles of reduction scratch,
// G (n columns of m | 1), V (n columns of n | 1; jobu only), the singular values
// and the signs (2 n), the inverse of the ranks (n ints), the flag word (padded
// to 16 bytes).
__host__ __device__ inline size_t lds_bytes(int esize, i64 m, i64 n, int jobu = 1) {
  return (size_t)MAX_WAVES * 8 + (size_t)(n * (m | 1) + (jobu ? n * (n | 1) : 0) + 2 * n) * esize + (size_t)n * 4 + 16;
}

// The largest multiple of 32 for which a square matrix fits: 128 (float32), 96 (float64).
inline i64 nmax_of(int esize) {
  i64 n = 32;
  while (lds_bytes(esize, n + 32, n + 32) <= (size_t)LDS_BYTES) n += 32;
  return n;
}

// The largest m that fits beside n columns (and, for jobu, an n x n V); 0 where
// not even m = n does.
inline i64 mmax_of(int esize, i64 n, int jobu = 1) {
  if (n < 1 || n > nmax_of(esize) || lds_bytes(esize, n, n, jobu) > (size_t)LDS_BYTES) return 0;
  const i64 rest = (i64)LDS_BYTES - (i64)lds_bytes(esize, 0, n, jobu);  // what G's columns may take beyond one entry each
  const i64 stride = rest / (n * esize) + 1;                            // the largest column stride
  return (stride & 1) ? stride : stride - 1;  // an even m needs the stride m + 1
}

// Lanes per pair (a power of two within a wave) and the workgroup size, from
// (m, n) alone.  Both phases of a round are bound by 4- / 8-byte LDS traffic,
// which a CU serves at its full rate only with several waves on every SIMD (the
// measurement quoted in eigh_kernels.h), so the pairs take as many lanes as the
// 1024 threads allow, but no more than half of them would find a row.
inline int lp_log2_of(i64 m, i64 n) {
  const i64 npairs = (n + 1) >> 1;
  int lg = 6;
  while (lg > 0 && (((i64)1 << lg) * npairs > 1024 || ((i64)1 << (lg - 1)) >= m)) --lg;
  return lg;
}
inline int threads_of(i64 m, i64 n) {
  const i64 want = ((n + 1) >> 1) << lp_log2_of(m, n);
  const i64 nt = (want + 63) / 64 * 64;
  return (int)(nt < 64 ? 64 : nt > 1024 ? 1024 : nt);
}

template <typename T>
__device__ inline void fill_nan(int jobu, T* __restrict__ Ub, i64 ldu, T* __restrict__ Sb, T* __restrict__ Vb, i64 ldvt,
                                int m, int n, int tid, int nt) {
  const T nan = std::numeric_limits<T>::quiet_NaN();
  for (int j = tid; j < n; j += nt) Sb[j] = nan;
  if (!jobu) return;
  for (int idx = tid; idx < m * n; idx += nt) {
    const int i = idx / n, c = idx - i * n;
    Ub[(i64)i * ldu + c] = nan;
  }
  for (int idx = tid; idx < n * n; idx += nt) {
    const int i = idx / n, c = idx - i * n;
    Vb[(i64)i * ldvt + c] = nan;
  }
}

template <typename T>
__global__ __launch_bounds__(1024) void k_gesvj(int jobu, int m, int n, int lp_log2, const T* __restrict__ A, i64 lda,
                                               i64 stride_a, T* __restrict__ U, i64 ldu, i64 stride_u,
                                               T* __restrict__ Sv, i64 stride_s, T* __restrict__ Vt, i64 ldvt,
                                               i64 stride_vt, int32_t* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) unsigned char svd_smem[];
  const int MS = m | 1, NS = n | 1, mm = n + (n & 1), npairs = mm >> 1;
  double* red = (double*)svd_smem;
  T* g = (T*)(red + MAX_WAVES);
  T* v = g + n * MS;
  T* sv = v + (jobu ? n * NS : 0);
  T* sg = sv + n;
  int* inv = (int*)(sg + n);
  int* flag = inv + n;
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  // LP = 2^lp_log2 lanes own one pair (or, in the finish, one column)
  const int LP = 1 << lp_log2, sub = tid & (LP - 1), grp = tid >> lp_log2, ngroups = nt >> lp_log2;
  const i64 b = blockIdx.x;
  const T* Ab = A + b * stride_a;
  T* Ub = jobu ? U + b * stride_u : nullptr;
  T* Sb = Sv + b * stride_s;
  T* Vb = jobu ? Vt + b * stride_vt : nullptr;

  // ---- load: G = A, V = I, the largest magnitude (inf: not finite)
  T amax = 0;
  for (int idx = tid; idx < m * n; idx += nt) {
    const int i = idx / n, j = idx - i * n;
    const T x = Ab[(i64)i * lda + j];
    g[j * MS + i] = x;
    const T ax = fabs(x);
    amax = fmax(amax, ax <= std::numeric_limits<T>::max() ? ax : std::numeric_limits<T>::infinity());
  }
  if (jobu)
    for (int idx = tid; idx < n * n; idx += nt) {
      const int i = idx / n, j = idx - i * n;
      v[j * NS + i] = i == j ? (T)1 : (T)0;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o, 64));
  if (lane == 0) red[wave] = (double)amax;
  __syncthreads();
  double big = 0;
  for (int w = 0; w < nw; ++w) big = fmax(big, red[w]);
  if (big == 0) {  // (uniform: every thread read the same words)
    for (int j = tid; j < n; j += nt) Sb[j] = 0;
    if (jobu) {
      for (int idx = tid; idx < m * n; idx += nt) {
        const int i = idx / n, c = idx - i * n;
        Ub[(i64)i * ldu + c] = 0;
      }
      for (int idx = tid; idx < n * n; idx += nt) {
        const int i = idx / n, c = idx - i * n;
        Vb[(i64)i * ldvt + c] = i == c ? (T)1 : (T)0;
      }
    }
    if (tid == 0) info[b] = 0;
    return;
  }
  if (!(big <= (double)std::numeric_limits<T>::max())) {
    fill_nan(jobu, Ub, ldu, Sb, Vb, ldvt, m, n, tid, nt);
    if (tid == 0) info[b] = -1;
    return;
  }

  // ---- scale by the power of two of the largest magnitude (exact)
  const int e = ilogb((T)big);
  for (int j = grp; j < n; j += ngroups) {
    T* col = g + j * MS;
    for (int i = sub; i < m; i += LP) col[i] = ldexp(col[i], -e);
  }
  const T tol = (T)(sqrt((double)m) * Eps<T>::u);
  // A column whose squared norm is at most the smallest normal number / u counts as a zero column, in the
  // rounds and in the finish: below that the three sums lose their relative accuracy to gradual underflow and
  // the test of a pair means nothing.  (The scaled matrix has its largest entry in [1, 2): such a column is
  // below 5e-16 (float32) / 2e-146 (float64) of it.)
  const T tiny = (T)((double)std::numeric_limits<T>::min() / Eps<T>::u);

  // ---- the sweeps
  int sweeps = 0;
  bool converged = n == 1;  // no pair: nothing to do
  if (n > 1) {
    for (int sweep = 0; sweep < SWEEP_MAX; ++sweep) {
      if (tid == 0) flag[0] = 0;
      __syncthreads();  // the reset (and, in the first sweep, the scaling), before any round
      for (int r = 0; r < mm - 1; ++r) {
        for (int k = grp; k < npairs; k += ngroups) {
          int p, q;
          pair_of(k, r, mm, p, q);
          if (q >= n) continue;  // the phantom's pair idles
          T* gp = g + p * MS;
          T* gq = g + q * MS;
          T app = 0, aqq = 0, apq = 0;
          for (int i = sub; i < m; i += LP) {
            const T x = gp[i], y = gq[i];
            app += x * x;
            aqq += y * y;
            apq += x * y;
          }
          for (int o = LP >> 1; o > 0; o >>= 1) {  // a butterfly: the same bits in every lane of the group
            app += __shfl_xor(app, o, 64);
            aqq += __shfl_xor(aqq, o, 64);
            apq += __shfl_xor(apq, o, 64);
          }
          if (!(app > tiny && aqq > tiny && fabs(apq) > tol * sqrt(app) * sqrt(aqq))) continue;
          const T theta = (aqq - app) / (2 * apq), at = fabs(theta);
          // from 1 / u on, theta^2 + 1 rounds to theta^2 and the formula gives 1 / (2 |theta|) bit for bit:
          // written out, so that theta^2 cannot overflow (a tiny column parallel to a large one gets there)
          T t = at >= (T)(1 / Eps<T>::u) ? 1 / (2 * at) : 1 / (at + sqrt(at * at + 1));
          if (theta < 0) t = -t;
          const T c = 1 / sqrt(t * t + 1);
          const T s = t * c;
          if (sub == 0) flag[0] = 1;  // a plain store of the same value by every rotating pair
          for (int i = sub; i < m; i += LP) {
            const T x = gp[i], y = gq[i];
            gp[i] = c * x - s * y;
            gq[i] = s * x + c * y;
          }
          if (jobu) {
            T* vp = v + p * NS;
            T* vq = v + q * NS;
            for (int i = sub; i < n; i += LP) {
              const T x = vp[i], y = vq[i];
              vp[i] = c * x - s * y;
              vq[i] = s * x + c * y;
            }
          }
        }
        __syncthreads();  // the round's one barrier: the next round pairs the columns anew
      }
      const int rotated = flag[0];  // after the round's barrier: the same word for every thread
      __syncthreads();              // this read, before the next sweep's reset
      sweeps = sweep + 1;
      if (!rotated) {
        converged = true;
        break;
      }
    }
  } else {
    __syncthreads();  // the scaling, before the finish reads other lanes' rows
  }
  if (!converged) {
    fill_nan(jobu, Ub, ldu, Sb, Vb, ldvt, m, n, tid, nt);
    if (tid == 0) info[b] = -1;
    return;
  }

  // ---- finish: singular values (scaled), signs, ranks, the permuted store
  for (int j = grp; j < n; j += ngroups) {
    const T* col = g + j * MS;
    double ss = 0;
    for (int i = sub; i < m; i += LP) {
      const double x = (double)col[i];
      ss += x * x;
    }
    for (int o = LP >> 1; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (sub == 0) sv[j] = ss > (double)tiny ? (T)sqrt(ss) : (T)0;
  }
  if (jobu)
    for (int j = tid; j < n; j += nt) {
      const T* col = v + j * NS;
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
  for (int j = tid; j < n; j += nt) {
    const T sj = sv[j];
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
      const T si = sv[i];
      cnt += (si > sj || (si == sj && i < j)) ? 1 : 0;
    }
    inv[cnt] = j;
    Sb[cnt] = ldexp(sj, e);
  }
  if (jobu) {
    __syncthreads();
    for (int idx = tid; idx < m * n; idx += nt) {
      const int i = idx / n, c = idx - i * n;
      const int j = inv[c];
      const T sj = sv[j];
      Ub[(i64)i * ldu + c] = sj > 0 ? sg[j] * (g[j * MS + i] / sj) : (T)0;
    }
    for (int idx = tid; idx < n * n; idx += nt) {
      const int c = idx / n, i = idx - c * n;
      const int j = inv[c];
      Vb[(i64)c * ldvt + i] = sg[j] * v[j * NS + i];
    }
  }
  if (tid == 0) info[b] = sweeps;
}

template <typename T>
static hipError_t run(int jobu, i64 batch, i64 m, i64 n, const T* A, i64 lda, i64 stride_a, T* U, i64 ldu, i64 stride_u,
                      T* Sv, i64 stride_s, T* Vt, i64 ldvt, i64 stride_vt, int32_t* info, hipStream_t s) {
  const size_t lds = lds_bytes(sizeof(T), m, n, jobu);
  hipError_t e = hipFuncSetAttribute((const void*)k_gesvj<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_gesvj<T>), dim3((unsigned)batch), dim3(threads_of(m, n)), lds, s, jobu, (int)m, (int)n,
                     lp_log2_of(m, n), A, lda, stride_a, U, ldu, stride_u, Sv, stride_s, Vt, ldvt, stride_vt, info);
  return hipGetLastError();
}

}  // namespace spx_svd

// ------------------------------------------------------------------ C ABI
extern "C" int spx_gesvj_plan(int dtype, int64_t n, int64_t* nmax, int64_t* mmax, int64_t* sweep_max) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_gesvj_plan: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_gesvj_plan: dtype %d is not float32 / float64", dtype);
  if (n < 0) return set_err(SPX_EINVAL, "spx_gesvj_plan: negative n = %lld", (long long)n);
  const int es = dtype == SPX_F32 ? 4 : 8;
  if (nmax) *nmax = spx_svd::nmax_of(es);
  if (mmax) *mmax = spx_svd::mmax_of(es, n, 1);
  if (sweep_max) *sweep_max = spx_svd::SWEEP_MAX;
  return SPX_OK;
}

extern "C" int spx_gesvj(int dtype, int jobu, int64_t batch, int64_t m, int64_t n, const void* A, int64_t lda,
                         int64_t stride_a, void* U, int64_t ldu, int64_t stride_u, void* S_, int64_t stride_s, void* Vt,
                         int64_t ldvt, int64_t stride_vt, int32_t* info, void* stream) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_gesvj: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_gesvj: dtype %d is not float32 / float64", dtype);
  if (jobu != 0 && jobu != 1) return set_err(SPX_EINVAL, "spx_gesvj: jobu %d is not 0 (S only) or 1", jobu);
  if (batch < 0 || m < 0 || n < 0)
    return set_err(SPX_EINVAL, "spx_gesvj: negative size (batch %lld, m %lld, n %lld)", (long long)batch, (long long)m,
                   (long long)n);
  if (m < n) return set_err(SPX_EINVAL, "spx_gesvj: m = %lld is below n = %lld", (long long)m, (long long)n);
  const int es = dtype == SPX_F32 ? 4 : 8;
  if (n > spx_svd::nmax_of(es))
    return set_err(SPX_ENOTSUP, "spx_gesvj: n = %lld is above the limit %lld", (long long)n,
                   (long long)spx_svd::nmax_of(es));
  if (n > 0 && m > spx_svd::mmax_of(es, n, jobu))
    return set_err(SPX_ENOTSUP, "spx_gesvj: m = %lld is above the limit %lld for n = %lld", (long long)m,
                   (long long)spx_svd::mmax_of(es, n, jobu), (long long)n);
  if (batch > 0x7fffffffLL) return set_err(SPX_ENOTSUP, "spx_gesvj: batch = %lld is above 2^31 - 1", (long long)batch);
  if (batch == 0 || n == 0) return SPX_OK;
  if (!A || !S_ || !info || (jobu ? (!U || !Vt) : (U || Vt)))
    return set_err(SPX_EINVAL, "spx_gesvj: null pointer (U and Vt are NULL iff jobu == 0)");
  if (lda < n || (jobu && (ldu < n || ldvt < n)))
    return set_err(SPX_EINVAL, "spx_gesvj: leading dimension (lda %lld, ldu %lld, ldvt %lld) below n = %lld",
                   (long long)lda, (long long)ldu, (long long)ldvt, (long long)n);
  if (stride_a < 0) return set_err(SPX_EINVAL, "spx_gesvj: negative stride_a %lld", (long long)stride_a);
  if (batch > 1 &&
      (stride_s < n || (jobu && (stride_u < (m - 1) * ldu + n || stride_vt < (n - 1) * ldvt + n))))
    return set_err(SPX_EINVAL,
                   "spx_gesvj: output strides (stride_u %lld, stride_s %lld, stride_vt %lld) let matrices overlap",
                   (long long)stride_u, (long long)stride_s, (long long)stride_vt);
  hipError_t e = dtype == SPX_F32
                     ? spx_svd::run<float>(jobu, batch, m, n, (const float*)A, lda, stride_a, (float*)U, ldu, stride_u,
                                           (float*)S_, stride_s, (float*)Vt, ldvt, stride_vt, info, S(stream))
                     : spx_svd::run<double>(jobu, batch, m, n, (const double*)A, lda, stride_a, (double*)U, ldu,
                                            stride_u, (double*)S_, stride_s, (double*)Vt, ldvt, stride_vt, info,
                                            S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_gesvj failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

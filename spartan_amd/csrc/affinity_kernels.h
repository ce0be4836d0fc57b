// Pairwise kernels of two point sets: spx_pairwise_plan / spx_pairwise
// (include/spx.h).  Included from spx.hip after nbody_kernels.h.
//
// For X (n, d) and Y (m, d), row-major, with s_ij = sum_k (x_ik - y_jk)^2:
//
//   sqeuclidean s_ij, euclidean sqrt(s_ij), manhattan sum_k |x_ik - y_jk|,
//   rbf exp(-gamma s_ij),
//
// optionally scaled by (r_i c_j), stored to out (n, m) with an optional
// diagonal override, and / or summed along each row.  One kernel serves the
// two passes of the reference's spectral-clustering Laplacian
// (spartan/examples/spectral_clustering.py): the degree pass (row sums only,
// nothing stored) and the pass that stores D^-1/2 A D^-1/2.
//
// The difference form only, never |x|^2 + |y|^2 - 2 x.y: every element runs
// k = 0 .. d - 1 in one order with one subtraction and one fused multiply-add
// (manhattan: one subtraction, one add of the absolute value) each, so equal
// rows give exactly 0 and (x_i - x_j)^2 == (x_j - x_i)^2 makes Y = X bitwise
// symmetric.  No MFMA form has either property.
//
// k_pairwise: 256 threads, a TB x TB = 64 x 64 tile of pairs, a 4 x 4
// micro-tile per lane (graph_kernels.h' minplus_tile with (-, fma) for
// (+, min)).  A workgroup owns TB rows of X and one of `splits` column ranges
// (blockIdx.y), and walks the range's column tiles in ascending order.  Per
// tile the operands pass through LDS KC = 16 values of k at a time: X rows as
// As[TB][KC + V] (V = 16 bytes of elements), Y rows TRANSPOSED as Bs[KC][TB].
// A lane (ty, tx) = (tid / 16, tid % 16) holds rows 4 ty + r and columns
// (c / V) 16 V + tx V + c % V.  Bank rules as in graph_kernels.h: the A read is
// one 16-byte address per ty, broadcast over tx, and the row pad keeps the two
// ty of a 16-lane group 16 banks apart; the B read of a group's 16 tx is one
// contiguous 256-byte line.  The transposing stage writes consecutive lanes to
// consecutive columns of one Bs row.  Rows, columns and k past the edge are
// zero in LDS ((0 - 0)^2 adds an exact 0) and masked at the store and the sum.
// When d <= KC the X chunk is staged once for the whole walk.
//
// Row sums: a lane adds the (at most four) values of its columns of a tile in
// T and adds that to a float64 accumulator per row, carried across the tiles;
// after the walk the 16 lanes of a row are added in a fixed xor-shuffle order.
// splits == 1 stores them as T; otherwise as float64 partials [split][n] that
// k_pairwise_sum adds in ascending split order.  No atomics; the same inputs
// and split give the same bits.
//
// float32 rbf is v_exp_f32 of (-gamma s) log2(e): DESIGN.md 3.27 has the error
// account.  float64 calls the device library's exp.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace spx_affinity {

typedef int64_t i64;

constexpr int TB = 64;           // tile edge: rows a workgroup owns, columns per step of its walk
constexpr int NT = 256;          // threads of a workgroup
constexpr int MT = 4;            // micro-tile edge
constexpr int KC = 16;           // values of k staged at a time
constexpr int RANGE_MIN = 4;     // the planner's shortest column range, in tiles
constexpr i64 SPLITS_MAX = 1024; // column ranges (grid.y)

template <typename T>
struct Vec;
template <>
struct Vec<float> {
  typedef float4 type;
  static constexpr int V = 4;
};
template <>
struct Vec<double> {
  typedef double2 type;
  static constexpr int V = 2;
};

__device__ __forceinline__ float vget(const float4& v, int i) {
  return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}
__device__ __forceinline__ double vget(const double2& v, int i) { return i == 0 ? v.x : v.y; }
__device__ __forceinline__ float4 vmake(const float* p) { return make_float4(p[0], p[1], p[2], p[3]); }
__device__ __forceinline__ double2 vmake(const double* p) { return make_double2(p[0], p[1]); }

__device__ __forceinline__ float fmad(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fmad(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float absv(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ double absv(double a) { return __builtin_fabs(a); }
__device__ __forceinline__ float sqrtv(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double sqrtv(double a) { return __builtin_sqrt(a); }
// exp(-g s), s >= 0 or NaN.  float32: one multiply by -g, one by log2(e), the hardware exp2.
__device__ __forceinline__ float rbfv(float s, float g) {
  return __builtin_amdgcn_exp2f((-g * s) * 1.44269504088896341f);
}
__device__ __forceinline__ double rbfv(double s, double g) { return exp(-g * s); }

// column c (0 .. 3) of lane tx's micro-tile
template <typename T>
__device__ __forceinline__ int col_of(int tx, int c) {
  constexpr int V = Vec<T>::V;
  return (c / V) * (16 * V) + tx * V + (c % V);
}

// Rows row0 .. row0 + TB of P (rows x d, leading dimension ld), columns
// kc .. kc + KC, into LDS; zero outside the matrix.  TRANSPOSED = false:
// dst[r][KC + V]; true: dst[k][TB].  16-byte global loads where `vec` (base
// and leading dimension 16-byte aligned) and the vector lies inside the row.
template <typename T, bool TRANSPOSED>
__device__ __forceinline__ void stage(T* __restrict__ dst, const T* __restrict__ P, i64 ld, i64 rows, i64 d, i64 row0,
                                      i64 kc, bool vec, int tid) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::V, VPR = KC / V, LDA = KC + V;
  static_assert((TB * VPR) % NT == 0, "a whole number of vectors per thread");
#pragma unroll
  for (int it = 0; it < TB * VPR / NT; ++it) {
    const int idx = it * NT + tid;
    // (transposed: consecutive lanes on consecutive rows, so the LDS writes of a k are one line)
    const int r = TRANSPOSED ? idx % TB : idx / VPR, kv = (TRANSPOSED ? idx / TB : idx % VPR) * V;
    const i64 gr = row0 + r, gk = kc + kv;
    T e[V];
    if (gr < rows && vec && gk + V <= d) {
      const VT v = *(const VT*)(P + gr * ld + gk);
#pragma unroll
      for (int q = 0; q < V; ++q) e[q] = vget(v, q);
    } else {
#pragma unroll
      for (int q = 0; q < V; ++q) e[q] = (gr < rows && gk + q < d) ? P[gr * ld + gk + q] : (T)0;
    }
    if (TRANSPOSED) {
#pragma unroll
      for (int q = 0; q < V; ++q) dst[(kv + q) * TB + r] = e[q];
    } else {
      *(VT*)(dst + r * LDA + kv) = vmake(e);
    }
  }
}

enum {  // the metric codes of include/spx.h
  M_SQEUCLIDEAN = SPX_PAIR_SQEUCLIDEAN,
  M_EUCLIDEAN = SPX_PAIR_EUCLIDEAN,
  M_MANHATTAN = SPX_PAIR_MANHATTAN,
  M_RBF = SPX_PAIR_RBF,
  M_COUNT = 4
};
static_assert(M_SQEUCLIDEAN == 0 && M_EUCLIDEAN == 1 && M_MANHATTAN == 2 && M_RBF == 3,
              "the codes are 0 .. M_COUNT - 1");

// acc += over KC values of k; As [TB][KC + V], Bs [KC][TB]
template <typename T, int METRIC>
__device__ __forceinline__ void pair_tile(T (&acc)[MT][MT], const T* __restrict__ As, const T* __restrict__ Bs, int ty,
                                          int tx) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::V, LDA = KC + V;
  // 8 / 2 values of k an iteration: unrolled whole, the compiler reads a chunk's operands ahead into 150 - 220
  // registers (two or three waves a SIMD); so it stays within 128 (four)
  constexpr int UNROLL = V == 4 ? 2 : 1;
#pragma unroll UNROLL
  for (int k0 = 0; k0 < KC; k0 += V) {
    VT a[MT];
#pragma unroll
    for (int r = 0; r < MT; ++r) a[r] = *(const VT*)(As + (ty * MT + r) * LDA + k0);
#pragma unroll
    for (int kk = 0; kk < V; ++kk) {
      VT b[MT / V];
#pragma unroll
      for (int g = 0; g < MT / V; ++g) b[g] = *(const VT*)(Bs + (k0 + kk) * TB + g * (16 * V) + tx * V);
#pragma unroll
      for (int r = 0; r < MT; ++r)
#pragma unroll
        for (int c = 0; c < MT; ++c) {
          const T df = vget(a[r], kk) - vget(b[c / V], c % V);
          acc[r][c] = METRIC == M_MANHATTAN ? acc[r][c] + absv(df) : fmad(df, df, acc[r][c]);
        }
    }
  }
}

template <typename T, int METRIC>
__global__ __launch_bounds__(NT) void k_pairwise(i64 n, i64 m, i64 d, const T* __restrict__ X, i64 ldx,
                                                 const T* __restrict__ Y, i64 ldy, T gamma, T* __restrict__ out,
                                                 i64 ldo, T* __restrict__ row_sums, double* __restrict__ part,
                                                 const T* __restrict__ row_scale, const T* __restrict__ col_scale,
                                                 i64 diag_col0, T diag_value, i64 per_split, int vecx, int vecy,
                                                 int veco) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::V;
  __shared__ __attribute__((aligned(16))) T As[TB * (KC + V)];
  __shared__ __attribute__((aligned(16))) T Bs[KC * TB];
  const int tid = (int)threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const i64 row0 = (i64)blockIdx.x * TB;
  const i64 cbeg = (i64)blockIdx.y * per_split;  // (a multiple of TB)
  const i64 cend = cbeg + per_split < m ? cbeg + per_split : m;  // (may be <= cbeg: an empty range)
  const bool sums = row_sums != nullptr || part != nullptr;
  const bool one_chunk = d <= KC;

  T rs[MT];
  double racc[MT];
#pragma unroll
  for (int r = 0; r < MT; ++r) {
    const i64 gr = row0 + ty * MT + r;
    rs[r] = (row_scale && gr < n) ? row_scale[gr] : (T)1;
    racc[r] = 0.0;
  }

#pragma unroll 1
  for (i64 col0 = cbeg; col0 < cend; col0 += TB) {
    T acc[MT][MT];
#pragma unroll
    for (int r = 0; r < MT; ++r)
#pragma unroll
      for (int c = 0; c < MT; ++c) acc[r][c] = (T)0;
#pragma unroll 1
    for (i64 kc = 0; kc < d; kc += KC) {
      __syncthreads();  // the chunk before has been read by every wave
      if (!one_chunk || col0 == cbeg) stage<T, false>(As, X, ldx, n, d, row0, kc, vecx != 0, tid);
      stage<T, true>(Bs, Y, ldy, m, d, col0, kc, vecy != 0, tid);
      __syncthreads();
      pair_tile<T, METRIC>(acc, As, Bs, ty, tx);
    }

    // the epilogue: metric, scales, row sums, diagonal, store
    T cs[MT];
#pragma unroll
    for (int c = 0; c < MT; ++c) {
      const i64 gc = col0 + col_of<T>(tx, c);
      cs[c] = (col_scale && gc < m) ? col_scale[gc] : (T)1;
    }
#pragma unroll
    for (int r = 0; r < MT; ++r) {
      const i64 gr = row0 + ty * MT + r;
      T v[MT];
#pragma unroll
      for (int c = 0; c < MT; ++c) {
        T a = acc[r][c];
        if (METRIC == M_EUCLIDEAN) a = sqrtv(a);
        if (METRIC == M_RBF) a = rbfv(a, gamma);
        if (row_scale) a = a * (rs[r] * cs[c]);  // the product of the scales first: symmetric for r == c
        v[c] = a;
      }
      if (sums) {
        T t = (T)0;  // columns past m add nothing; the order is c = 0 .. 3
#pragma unroll
        for (int c = 0; c < MT; ++c) t += (col0 + col_of<T>(tx, c) < m) ? v[c] : (T)0;
        racc[r] += (double)t;
      }
      if (out && gr < n) {
        if (diag_col0 >= 0) {
          const i64 dc = diag_col0 + gr;
#pragma unroll
          for (int c = 0; c < MT; ++c)
            if (col0 + col_of<T>(tx, c) == dc) v[c] = diag_value;
        }
#pragma unroll
        for (int g = 0; g < MT / V; ++g) {
          const i64 gc = col0 + col_of<T>(tx, g * V);
          if (veco && gc + V <= m) {
            *(VT*)(out + gr * ldo + gc) = vmake(&v[g * V]);
          } else {
#pragma unroll
            for (int q = 0; q < V; ++q)
              if (gc + q < m) out[gr * ldo + gc + q] = v[g * V + q];
          }
        }
      }
    }
  }

  if (sums) {
#pragma unroll
    for (int r = 0; r < MT; ++r) {
      double t = racc[r];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) t += __shfl_xor(t, off, 16);
      const i64 gr = row0 + ty * MT + r;
      if (tx == 0 && gr < n) {
        if (part)
          part[(i64)blockIdx.y * n + gr] = t;
        else
          row_sums[gr] = (T)t;
      }
    }
  }
}

// row_sums[i] = sum over the splits, in ascending order, of part[s][i]
template <typename T>
__global__ __launch_bounds__(NT) void k_pairwise_sum(i64 n, i64 splits, const double* __restrict__ part,
                                                     T* __restrict__ row_sums) {
  const i64 i = (i64)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  double a = 0.0;
  for (i64 s = 0; s < splits; ++s) a += part[s * n + i];
  row_sums[i] = (T)a;
}

// ------------------------------------------------------------------- plan
// The column ranges: enough workgroups for four per CU, no range shorter than
// RANGE_MIN tiles, never more than SPLITS_MAX.  Pure arithmetic.
static i64 plan_splits(i64 n, i64 m, i64 cus) {
  if (n < 1 || m < 1) return 1;
  const i64 blocks = (n + TB - 1) / TB, tiles = (m + TB - 1) / TB, most = (tiles + RANGE_MIN - 1) / RANGE_MIN;
  i64 s = (4 * cus + blocks - 1) / blocks;
  if (s > most) s = most;
  if (s > SPLITS_MAX) s = SPLITS_MAX;
  return s < 1 ? 1 : s;
}

// the columns of one range: whole tiles (the trailing ranges of a forced split may be empty)
static i64 per_split_of(i64 m, i64 splits) {
  const i64 tiles = (m + TB - 1) / TB;
  return (tiles + splits - 1) / splits * TB;
}

static i64 workspace_for(i64 n, i64 splits) { return splits > 1 ? splits * n * 8 : 0; }

static bool aligned16(const void* p, i64 ld, size_t esz) {
  return p && (uintptr_t)p % 16 == 0 && ((size_t)ld * esz) % 16 == 0;
}

template <typename T>
static hipError_t run(int metric, i64 n, i64 m, i64 d, const T* X, i64 ldx, const T* Y, i64 ldy, double gamma, T* out,
                      i64 ldo, T* row_sums, const T* row_scale, const T* col_scale, i64 diag_col0, double diag_value,
                      i64 splits, double* part, hipStream_t s) {
  const i64 blocks = (n + TB - 1) / TB, per = per_split_of(m, splits);
  const bool split_sums = row_sums && splits > 1;
  const dim3 grid((unsigned)blocks, (unsigned)splits);
  const int vx = aligned16(X, ldx, sizeof(T)), vy = aligned16(Y, ldy, sizeof(T)), vo = aligned16(out, ldo, sizeof(T));
#define SPX_PAIRWISE_LAUNCH(M)                                                                                        \
  k_pairwise<T, M><<<grid, NT, 0, s>>>(n, m, d, X, ldx, Y, ldy, (T)gamma, out, ldo, split_sums ? nullptr : row_sums,  \
                                       split_sums ? part : nullptr, row_scale, col_scale, diag_col0, (T)diag_value,  \
                                       per, vx, vy, vo)
  switch (metric) {
    case M_SQEUCLIDEAN: SPX_PAIRWISE_LAUNCH(M_SQEUCLIDEAN); break;
    case M_EUCLIDEAN: SPX_PAIRWISE_LAUNCH(M_EUCLIDEAN); break;
    case M_MANHATTAN: SPX_PAIRWISE_LAUNCH(M_MANHATTAN); break;
    default: SPX_PAIRWISE_LAUNCH(M_RBF); break;
  }
#undef SPX_PAIRWISE_LAUNCH
  if (split_sums) k_pairwise_sum<T><<<(unsigned)((n + NT - 1) / NT), NT, 0, s>>>(n, splits, part, row_sums);
  return hipGetLastError();
}

}  // namespace spx_affinity

// ------------------------------------------------------------------ C ABI
static int pairwise_check(const char* who, int dtype, int64_t n, int64_t m, int64_t splits) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "%s: bad dtype %d", who, dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "%s: dtype %d is not float32 / float64", who, dtype);
  if (n < 0 || m < 0) return set_err(SPX_EINVAL, "%s: negative size (n %lld, m %lld)", who, (long long)n, (long long)m);
  if (n > (int64_t)spx_affinity::TB * 0x7fffffffLL)
    return set_err(SPX_ENOTSUP, "%s: n = %lld is above the grid limit", who, (long long)n);
  if (m > (1LL << 48)) return set_err(SPX_ENOTSUP, "%s: m = %lld is above the limit 2^48", who, (long long)m);
  if (splits < 0 || splits > spx_affinity::SPLITS_MAX)
    return set_err(SPX_EINVAL, "%s: splits = %lld is outside 0 .. %lld", who, (long long)splits,
                   (long long)spx_affinity::SPLITS_MAX);
  return SPX_OK;
}

extern "C" int spx_pairwise_plan(int dtype, int64_t n, int64_t m, int64_t* tile, int64_t* k_chunk, int64_t* splits,
                                 size_t* workspace_bytes) {
  if (tile) *tile = spx_affinity::TB;
  if (k_chunk) *k_chunk = spx_affinity::KC;
  const int64_t forced = splits ? *splits : 0;
  int rc = pairwise_check("spx_pairwise_plan", dtype, n, m, forced);
  if (rc != SPX_OK) return rc;
  const int64_t use = forced > 0 ? forced : spx_affinity::plan_splits(n, m, num_cus());
  if (splits) *splits = use;
  if (workspace_bytes) *workspace_bytes = (size_t)spx_affinity::workspace_for(n, use);
  return SPX_OK;
}

extern "C" int spx_pairwise(int dtype, int metric, int64_t n, int64_t m, int64_t d, const void* X, int64_t ldx,
                            const void* Y, int64_t ldy, double gamma, void* out, int64_t ldo, void* row_sums,
                            const void* row_scale, const void* col_scale, int64_t diag_col0, double diag_value,
                            int64_t splits, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = pairwise_check("spx_pairwise", dtype, n, m, splits);
  if (rc != SPX_OK) return rc;
  if (metric < 0 || metric >= spx_affinity::M_COUNT)
    return set_err(SPX_EINVAL, "spx_pairwise: unknown metric %d", metric);
  if (d < 1) return set_err(SPX_EINVAL, "spx_pairwise: d = %lld < 1", (long long)d);
  if (!(gamma >= 0.0) || !std::isfinite(gamma))
    return set_err(SPX_EINVAL, "spx_pairwise: gamma = %g is not finite and >= 0", gamma);
  if (!out && !row_sums) return set_err(SPX_EINVAL, "spx_pairwise: out and row_sums are both NULL");
  if ((row_scale == nullptr) != (col_scale == nullptr))
    return set_err(SPX_EINVAL, "spx_pairwise: row_scale and col_scale go together (both or neither)");
  if (ldx < d || ldy < d) return set_err(SPX_EINVAL, "spx_pairwise: ldx = %lld / ldy = %lld is below d = %lld",
                                         (long long)ldx, (long long)ldy, (long long)d);
  if (out && ldo < m)
    return set_err(SPX_EINVAL, "spx_pairwise: ldo = %lld is below m = %lld", (long long)ldo, (long long)m);
  if (n == 0 || m == 0) return SPX_OK;
  if (!X || !Y) return set_err(SPX_EINVAL, "spx_pairwise: null pointer (X / Y)");
  const int64_t use = splits > 0 ? splits : spx_affinity::plan_splits(n, m, num_cus());
  const int64_t need = row_sums ? spx_affinity::workspace_for(n, use) : 0;
  if (need > 0) {
    if (!workspace || (int64_t)workspace_bytes < need)
      return set_err(SPX_EINVAL, "spx_pairwise: workspace %zu < %lld bytes for %lld splits", workspace_bytes,
                     (long long)need, (long long)use);
    if ((uintptr_t)workspace % 8 != 0) return set_err(SPX_EINVAL, "spx_pairwise: workspace is not 8-byte aligned");
  }
  hipError_t e =
      dtype == SPX_F32
          ? spx_affinity::run<float>(metric, n, m, d, (const float*)X, ldx, (const float*)Y, ldy, gamma, (float*)out,
                                     ldo, (float*)row_sums, (const float*)row_scale, (const float*)col_scale,
                                     diag_col0, diag_value, use, (double*)workspace, S(stream))
          : spx_affinity::run<double>(metric, n, m, d, (const double*)X, ldx, (const double*)Y, ldy, gamma,
                                      (double*)out, ldo, (double*)row_sums, (const double*)row_scale,
                                      (const double*)col_scale, diag_col0, diag_value, use, (double*)workspace,
                                      S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_pairwise failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

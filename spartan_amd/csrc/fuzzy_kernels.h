// Fuzzy k-means: spx_fuzzy_plan / spx_fuzzy_step.
// Included from spx.hip after graph_kernels.h.
//
// One pass over the points gives the soft assignment and the weighted centre
// sums.  Per row i, with d_j = |x_i - c_j|^2 + eps,
//
//   u_j = t_j / sum_j t_j,   t_j = (d_min / d_j)^exponent   (every t_j in (0, 1]),
//   sums[j, :] (+)= u_j^weight_power x_i,   counts[j] (+)= u_j^weight_power.
//
//   k_fuzzy_prep   the float64 centres -> the points' dtype, zero-padded to
//                  KMAX rows and a whole number of column panels (workspace);
//   k_fuzzy        one persistent workgroup per row group and column panel
//                  (grid (groups, panels); a panel is DP columns of the sums).
//                  A group walks its row tiles of RT rows in sub-tiles of RS:
//     distances    a lane owns one centre, held in DP registers; a wave owns
//                  a block of 64 centres and walks rows.  The row is wave-
//                  uniform: with one panel x is read from an LDS image of
//                  the sub-tile (every lane the same 16 bytes, a broadcast),
//                  with more panels through the scalar cache; the vector
//                  ALUs do (x - c)^2 in the difference form;
//     normalise    one wave per row over the distances in LDS: the first index
//                  of the minimum, the powers, their sum; labels and U leave
//                  for global memory, W = U^weight_power replaces the
//                  distances in LDS;
//     W^T X        on MFMA: wave w owns column tile w of the panel and every
//                  centre tile (A = W from LDS, B = X straight from global
//                  memory, loaded one sub-tile ahead so that it is there);
//                  the accumulators stay in registers over a whole row tile
//                  and are then added to this group's float64 partial;
//   k_kmeans_reduce  sums the groups' partials in a fixed order.
//
// float32 points: distances, memberships and the accumulators within one row
// tile are float32; the partials, the counts and their reduction float64.
// float64 points: float64 throughout.  No atomics; the same input gives the
// same bits.  No load is wider than an element, so any base address and any
// leading dimension take the same path.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace spx_fuzzy {

typedef int64_t i64;
using spx_mfma::Mfma;

constexpr int NT = 256;      // 4 waves
constexpr int RS = 32;       // rows of a sub-tile
constexpr int RT = 512;      // rows of a row tile: the float32 accumulators live this long
constexpr int KMAX = 256;    // one centre per lane of the workgroup
constexpr int POW_ANY = 0, POW_ONE = 1, POW_TWO = 2;

template <typename T>
struct Cfg;
template <>
struct Cfg<float> {
  static constexpr int DP = 128;  // columns of a panel: 4 waves x one 32-wide MFMA tile
};
template <>
struct Cfg<double> {
  static constexpr int DP = 64;   // 4 waves x one 16-wide MFMA tile
};

// row stride of the LDS image of W: the lane halves (float) / quarters (double)
// of an A-operand read are TILE elements apart, so they fall on disjoint banks
template <typename T>
constexpr int ldw_of() {
  return KMAX + Mfma<T>::TILE;
}
// row stride of the LDS image of the X sub-tile (rows stay 16-byte aligned)
template <typename T>
constexpr int ldx_of() {
  return Cfg<T>::DP + 16 / (int)sizeof(T);
}
template <typename T>
constexpr size_t lds_bytes() {
  return (size_t)RS * (ldw_of<T>() + ldx_of<T>()) * sizeof(T);
}

__device__ inline float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ inline double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// x^p for x in [0, 1].  float: exp2(p log2 x) on the hardware's 1-ulp units; the
// absolute error is at most |y| 2^y ln 2 2^-23 < 5e-8 for y = p log2 x.
__device__ inline float pow_t(float x, float p, int mode) {
  if (mode == POW_ONE) return x;
  if (mode == POW_TWO) return x * x;
  return __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(x));  // v_exp_f32 / v_log_f32 (base 2)
}
__device__ inline double pow_t(double x, double p, int mode) {
  if (mode == POW_ONE) return x;
  if (mode == POW_TWO) return x * x;
  return pow(x, p);
}

template <typename T>
__global__ __launch_bounds__(NT) void k_fuzzy_prep(i64 D, i64 K, i64 Dpad, const double* __restrict__ C,
                                                   T* __restrict__ Cw) {
  const i64 i = (i64)blockIdx.x * NT + threadIdx.x;
  if (i >= (i64)KMAX * Dpad) return;
  const i64 k = i / Dpad, d = i % Dpad;
  Cw[i] = (k < K && d < D) ? (T)C[k * D + d] : (T)0;
}

// sum over c (x_c - c_c)^2 for the DP columns from d0, four chains.  Not FULL:
// columns from D on count as zero (the padded centres are zero there); the
// index is clamped, so nothing past the row's D elements is read.
template <typename T, bool FULL>
__device__ inline T dist_chunk(const T* __restrict__ x, i64 d0, i64 D, const T (&c)[Cfg<T>::DP]) {
  constexpr int DP = Cfg<T>::DP;
  T a[4] = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    T xv;
    if (FULL) {
      xv = x[d0 + d];
    } else {
      const i64 at = d0 + d < D ? d0 + d : D - 1;
      xv = x[at];
      xv = d0 + d < D ? xv : (T)0;
    }
    const T t = xv - c[d];
    a[d & 3] = fma_t(t, t, a[d & 3]);
  }
  return (a[0] + a[1]) + (a[2] + a[3]);
}

// The same sum for a row held in LDS (zero from column D on, like the centres):
// every lane reads the same 16 bytes, which the LDS serves as a broadcast.
// Blocks of 32 columns from D on are skipped.  (A second copy without that test,
// whose reads run ahead across blocks, was tried: the two copies together spilled.)
template <typename T>
__device__ inline T dist_lds(const T* __restrict__ xs, i64 D, const T (&c)[Cfg<T>::DP]) {
  typedef typename Mfma<T>::vec_t vec_t;
  constexpr int DP = Cfg<T>::DP, V = 16 / (int)sizeof(T);
  T a[4] = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
  for (int blk = 0; blk < DP / 32; ++blk) {
    if (blk * 32 < D) {
#pragma unroll
      for (int d = blk * 32; d < blk * 32 + 32; d += V) {
        const vec_t v = *(const vec_t*)(xs + d);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const T t = v[e] - c[d + e];
          a[(d + e) & 3] = fma_t(t, t, a[(d + e) & 3]);
        }
      }
    }
  }
  return (a[0] + a[1]) + (a[2] + a[3]);
}

// MULTI: D is above one panel; the centres are then walked in chunks of DP
// columns (chunk outside, rows inside; the distances add up in LDS), and each
// column panel of the sums has a workgroup of its own that repeats the
// distances.  FULL (MULTI only): D is a whole number of chunks.
template <typename T, bool MULTI, bool FULL>
__global__ __launch_bounds__(NT) void k_fuzzy(i64 N, i64 D, i64 K, const T* __restrict__ P, i64 ldp,
                                              const T* __restrict__ Cw, i64 Dpad, T ex, T eps, T wp, int emode,
                                              int wmode, i64* __restrict__ labels, T* __restrict__ U, i64 ldu,
                                              double* __restrict__ psum, double* __restrict__ pcnt, i64 ntiles) {
  typedef Mfma<T> M;
  typedef typename M::acc_t acc_t;
  constexpr int DP = Cfg<T>::DP, TILE = M::TILE, KS = M::KS, KT = KMAX / TILE, LW = ldw_of<T>(), LX = ldx_of<T>();
  static_assert(DP == 4 * TILE, "one column tile a wave");
  extern __shared__ __attribute__((aligned(16))) unsigned char fuzzy_smem[];
  T* Ws = (T*)fuzzy_smem;
  T* Xs = Ws + RS * LW;  // the X sub-tile [RS][LX], not MULTI only

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int panel = blockIdx.y;
  const bool lead = panel == 0;  // the panel that writes labels, U and counts
  const i64 dcol = (i64)panel * DP + wave * TILE + M::opi(lane);  // this lane's column of X in the product
  const int nkb = (int)((K + 63) / 64);                           // blocks of 64 centres: 1 .. 4
  const int kbw = nkb >= 3 ? 4 : nkb;                             // waves across them: 1, 2, 4
  const int cb = wave % kbw, rphase = wave / kbw, rstep = 4 / kbw;
  const int myk = cb * 64 + lane;
  const int nkt = (int)((K + TILE - 1) / TILE);
  const int nchunk = (int)(Dpad / DP);
  const T inf = (T)__builtin_huge_val();
  const T* __restrict__ cw = Cw + (i64)myk * Dpad;

  T c[DP];
  if (!MULTI) {
#pragma unroll
    for (int d = 0; d < DP; ++d) c[d] = cw[d];
  }
  acc_t acc[KT];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) acc[kt] = M::zero();
  double cnt[4] = {0.0, 0.0, 0.0, 0.0};  // of centres lane + 64 i, over the rows this wave normalises
  // this workgroup's part of the group's partial: panel columns, zeroed here and added to below
  double* ps = psum + (i64)blockIdx.x * K * D;
  {
    const i64 c0 = (i64)panel * DP, cn = D - c0 < DP ? D - c0 : DP;
    for (i64 i = tid; i < K * cn; i += NT) ps[(i / cn) * D + c0 + i % cn] = 0.0;
  }
  __syncthreads();  // (workgroup-scope release / acquire: the zeros are seen by the lanes that add)

  // The sub-tiles of this group's row tiles, in order.  The B operand of the product (this lane's
  // column of X over the sub-tile's rows) is loaded one sub-tile ahead: it is there when the product
  // wants it, and it has brought the rows into L2 by the time the scalar loads of the distances ask.
  const auto load_b = [&](T (&b)[RS / KS], i64 r0) {
#pragma unroll
    for (int kk = 0; kk < RS / KS; ++kk) {
      const i64 row = r0 + kk * KS + M::opk(lane);
      b[kk] = (row < N && dcol < D) ? P[row * ldp + dcol] : (T)0;
    }
  };
  i64 t = blockIdx.x, r0 = t * RT;  // (the grid has no more groups than there are row tiles)
  T b[RS / KS], bn[RS / KS];
  load_b(b, r0);
#pragma unroll 1
  for (;;) {
    i64 nt = t, nr0 = r0 + RS;
    if (nr0 >= (t + 1) * RT || nr0 >= N) {
      nt = t + gridDim.x;
      nr0 = nt * RT;
    }
    const bool more = nt < ntiles;
    load_b(bn, more ? nr0 : N);  // (rows from N on load nothing)
    {
      // distances of the rows r0 .. r0 + RS to centre myk (rows past N: any finite value)
      if (!MULTI) {
        // one panel holds every column: the operand just loaded IS the sub-tile; through LDS it
        // reaches every lane (the scalar path below waits on memory three times a row)
#pragma unroll
        for (int kk = 0; kk < RS / KS; ++kk)
          Xs[(kk * KS + M::opk(lane)) * LX + wave * TILE + M::opi(lane)] = b[kk];
        __syncthreads();
      }
      if (cb < nkb) {
        if (!MULTI) {
#pragma unroll 1
          for (int r = rphase; r < RS; r += rstep) Ws[r * LW + myk] = dist_lds<T>(Xs + r * LX, D, c) + eps;
        } else {
#pragma unroll 1
          for (int ch = 0; ch < nchunk; ++ch) {
#pragma unroll
            for (int d = 0; d < DP; ++d) c[d] = cw[(i64)ch * DP + d];
            const bool whole = FULL || (i64)(ch + 1) * DP <= D;
#pragma unroll 1
            for (int r = rphase; r < RS; r += rstep) {
              const i64 row = r0 + r;
              T part = (T)0;
              if (row < N)
                part = whole ? dist_chunk<T, true>(P + row * ldp, (i64)ch * DP, D, c)
                             : dist_chunk<T, false>(P + row * ldp, (i64)ch * DP, D, c);
              Ws[r * LW + myk] = ch == 0 ? part + eps : Ws[r * LW + myk] + part;
            }
          }
        }
      }
      __syncthreads();
      // memberships: one wave a row
#pragma unroll 1
      for (int r = wave; r < RS; r += 4) {
        const i64 row = r0 + r;
        T dv[4];
        T best = inf;
        int bi = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = lane + 64 * i;
          dv[i] = j < K ? Ws[r * LW + j] : inf;
          if (dv[i] < best) {  // (j grows with i: the first of equals stays)
            best = dv[i];
            bi = j;
          }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          const T ob = __shfl_xor(best, off);
          const int oi = __shfl_xor(bi, off);
          if (ob < best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
          }
        }
        T tv[4];
        T sum = (T)0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          tv[i] = (lane + 64 * i) < K ? pow_t(best / dv[i], ex, emode) : (T)0;
          sum += tv[i];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);  // the same bits in every lane
        const bool live = row < N;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = lane + 64 * i;
          const T u = tv[i] / sum;
          T w = (T)0;
          if (live && j < K) {
            w = pow_t(u, wp, wmode);
            if (lead && U) U[row * ldu + j] = u;
            cnt[i] += (double)w;
          }
          Ws[r * LW + j] = w;
        }
        if (live && lead && labels && lane == 0) labels[row] = bi;
      }
      __syncthreads();
      // acc[kt] += W^T X: centre tile kt x this wave's column tile
#pragma unroll
      for (int kk = 0; kk < RS / KS; ++kk) {
        const int rr = kk * KS + M::opk(lane);
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
          if (kt < nkt) acc[kt] = M::mma(Ws[rr * LW + kt * TILE + M::opi(lane)], b[kk], acc[kt]);
      }
      __syncthreads();  // W has been read
    }
    // float32 accumulators end with the row tile; float64 ones with the group's last tile
    if (nt != t && (sizeof(T) == 4 || !more)) {
      const i64 col = (i64)panel * DP + wave * TILE + M::ccol(lane);
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        if (kt < nkt) {
          // the rows, masks and addresses are made here, from a lane number the optimiser cannot see
          // through: hoisted out of the row loops, the 128 of each would be live across the whole kernel
          int lq = lane;
          asm volatile("" : "+v"(lq));
#pragma unroll
          for (int q = 0; q < M::NREG; ++q) {
            const i64 k = kt * TILE + M::crow(lq, q);
            if (k < K && col < D) ps[k * D + col] += (double)acc[kt][q];
          }
          acc[kt] = M::zero();
          asm volatile("" ::: "memory");  // one centre tile's loads at a time: no more live registers than that
        }
      }
    }
    if (!more) break;
    t = nt;
    r0 = nr0;
#pragma unroll
    for (int kk = 0; kk < RS / KS; ++kk) b[kk] = bn[kk];
  }
  if (!lead) return;
  // counts: the four waves' shares, added in wave order
  double* cl = (double*)fuzzy_smem;  // [4][KMAX]; W is no longer read (the barrier above)
#pragma unroll
  for (int i = 0; i < 4; ++i) cl[wave * KMAX + lane + 64 * i] = cnt[i];
  __syncthreads();
  if (tid < K) pcnt[(i64)blockIdx.x * K + tid] = ((cl[tid] + cl[KMAX + tid]) + cl[2 * KMAX + tid]) + cl[3 * KMAX + tid];
}

struct Layout {
  i64 dpad, off_c, off_sum, off_cnt, bytes;
};

static i64 up256(i64 v) { return (v + 255) / 256 * 256; }

template <typename T>
static Layout layout(i64 D, i64 K, i64 G) {
  Layout l;
  l.dpad = (D + Cfg<T>::DP - 1) / Cfg<T>::DP * Cfg<T>::DP;
  l.off_c = 0;
  l.off_sum = up256((i64)KMAX * l.dpad * (i64)sizeof(T));
  l.off_cnt = l.off_sum + up256(G * K * D * 8);
  l.bytes = l.off_cnt + up256(G * K * 8);
  return l;
}

template <typename T>
static hipError_t run(i64 N, i64 D, i64 K, const T* P, i64 ldp, const double* C, double ex, double eps, double wp,
                      i64* labels, T* U, i64 ldu, double* sums, double* counts, int zero_first, char* ws, i64 G,
                      hipStream_t s) {
  const Layout l = layout<T>(D, K, G);
  T* Cw = (T*)(ws + l.off_c);
  double* psum = (double*)(ws + l.off_sum);
  double* pcnt = (double*)(ws + l.off_cnt);
  const i64 ntiles = (N + RT - 1) / RT, groups = ntiles < G ? ntiles : G, panels = l.dpad / Cfg<T>::DP;
  const i64 nprep = (i64)KMAX * l.dpad;
  hipLaunchKernelGGL((k_fuzzy_prep<T>), dim3((unsigned)((nprep + NT - 1) / NT)), dim3(NT), 0, s, D, K, l.dpad, C, Cw);
  constexpr size_t lds = lds_bytes<T>();
  static_assert(lds >= 4 * KMAX * sizeof(double), "the counts' exchange fits in W's image");
  typedef void (*kernel_t)(i64, i64, i64, const T*, i64, const T*, i64, T, T, T, int, int, i64*, T*, i64, double*, double*,
                           i64);
  const bool multi = panels > 1, full = D == l.dpad;
  const kernel_t kern = multi ? (full ? (kernel_t)k_fuzzy<T, true, true> : (kernel_t)k_fuzzy<T, true, false>)
                              : (kernel_t)k_fuzzy<T, false, true>;  // (one panel: FULL plays no part)
  if (lds > 48 * 1024) {  // set per call, as the attribute belongs to the current device
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const int emode = ex == 1.0 ? POW_ONE : ex == 2.0 ? POW_TWO : POW_ANY;
  const int wmode = wp == 1.0 ? POW_ONE : wp == 2.0 ? POW_TWO : POW_ANY;
  hipLaunchKernelGGL(kern, dim3((unsigned)groups, (unsigned)panels), dim3(NT), lds, s, N, D, K, P, ldp, (const T*)Cw,
                     l.dpad, (T)ex, (T)eps, (T)wp, emode, wmode, labels, U, ldu, psum, pcnt, ntiles);
  const i64 n = K * D;
  const int add = zero_first ? 0 : 1;
  k_kmeans_reduce<double><<<(unsigned)((n + 63) / 64), 256, 0, s>>>(n, groups, psum, sums, add);
  k_kmeans_reduce<double><<<(unsigned)((K + 63) / 64), 256, 0, s>>>(K, groups, pcnt, counts, add);
  return hipGetLastError();
}

constexpr i64 D_MAX = 1 << 20;  // columns (8192 panels and more: far past any use)

}  // namespace spx_fuzzy

// ------------------------------------------------------------------ C ABI
static int fuzzy_check_shape(const char* who, int dtype, int64_t N, int64_t D, int64_t K) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "%s: bad dtype %d", who, dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "%s: dtype %d is not float32 / float64", who, dtype);
  if (N < 0 || D < 1 || K < 1)
    return set_err(SPX_EINVAL, "%s: bad sizes (N %lld, D %lld, K %lld): N >= 0, D >= 1, K >= 1 are needed", who,
                   (long long)N, (long long)D, (long long)K);
  if (K > spx_fuzzy::KMAX)
    return set_err(SPX_ENOTSUP, "%s: K = %lld is above kmax = %d", who, (long long)K, spx_fuzzy::KMAX);
  if (D > spx_fuzzy::D_MAX)
    return set_err(SPX_ENOTSUP, "%s: D = %lld is above the limit %lld", who, (long long)D, (long long)spx_fuzzy::D_MAX);
  return SPX_OK;
}

extern "C" int spx_fuzzy_plan(int dtype, int64_t N, int64_t D, int64_t K, int64_t* row_tile, int64_t* groups,
                              int64_t* kmax, size_t* workspace_bytes) {
  if (kmax) *kmax = spx_fuzzy::KMAX;  // answered whatever K is: the caller's limit check reads it
  if (row_tile) *row_tile = spx_fuzzy::RT;
  const int64_t G = num_cus();
  if (groups) *groups = G;
  int rc = fuzzy_check_shape("spx_fuzzy_plan", dtype, N, D, K);
  if (rc != SPX_OK) return rc;
  if (workspace_bytes)
    *workspace_bytes = (size_t)(dtype == SPX_F32 ? spx_fuzzy::layout<float>(D, K, G).bytes
                                                 : spx_fuzzy::layout<double>(D, K, G).bytes);
  return SPX_OK;
}

extern "C" int spx_fuzzy_step(int dtype, int64_t N, int64_t D, int64_t K, const void* points, int64_t ldp,
                              const double* centers, double exponent, double eps, double weight_power,
                              int64_t* labels, void* U, int64_t ldu, double* sums, double* counts, int zero_first,
                              void* workspace, size_t workspace_bytes, void* stream) {
  int rc = fuzzy_check_shape("spx_fuzzy_step", dtype, N, D, K);
  if (rc != SPX_OK) return rc;
  if (!(exponent > 0.0) || !std::isfinite(exponent))
    return set_err(SPX_EINVAL, "spx_fuzzy_step: exponent = %g is not finite and > 0", exponent);
  if (!(eps > 0.0) || !std::isfinite(eps)) return set_err(SPX_EINVAL, "spx_fuzzy_step: eps = %g is not finite and > 0", eps);
  if (!(weight_power > 0.0) || !std::isfinite(weight_power))
    return set_err(SPX_EINVAL, "spx_fuzzy_step: weight_power = %g is not finite and > 0", weight_power);
  if (!sums || !counts) return set_err(SPX_EINVAL, "spx_fuzzy_step: null pointer (sums / counts)");
  if (N == 0) {
    if (zero_first) {
      HIP_TRY(hipMemsetAsync(sums, 0, (size_t)(K * D) * sizeof(double), S(stream)));
      HIP_TRY(hipMemsetAsync(counts, 0, (size_t)K * sizeof(double), S(stream)));
    }
    return SPX_OK;
  }
  if (!points || !centers) return set_err(SPX_EINVAL, "spx_fuzzy_step: null pointer (points / centers)");
  if (ldp < D) return set_err(SPX_EINVAL, "spx_fuzzy_step: ldp = %lld is below D = %lld", (long long)ldp, (long long)D);
  if (U && ldu < K) return set_err(SPX_EINVAL, "spx_fuzzy_step: ldu = %lld is below K = %lld", (long long)ldu, (long long)K);
  const int64_t G = num_cus();
  const int64_t need = dtype == SPX_F32 ? spx_fuzzy::layout<float>(D, K, G).bytes
                                        : spx_fuzzy::layout<double>(D, K, G).bytes;
  if (!workspace || (int64_t)workspace_bytes < need)
    return set_err(SPX_EINVAL, "spx_fuzzy_step: workspace %zu < %lld bytes", workspace_bytes, (long long)need);
  if ((uintptr_t)workspace % 16 != 0) return set_err(SPX_EINVAL, "spx_fuzzy_step: workspace is not 16-byte aligned");
  hipError_t e =
      dtype == SPX_F32
          ? spx_fuzzy::run<float>(N, D, K, (const float*)points, ldp, centers, exponent, eps, weight_power, labels,
                                  (float*)U, ldu, sums, counts, zero_first, (char*)workspace, G, S(stream))
          : spx_fuzzy::run<double>(N, D, K, (const double*)points, ldp, centers, exponent, eps, weight_power, labels,
                                   (double*)U, ldu, sums, counts, zero_first, (char*)workspace, G, S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_fuzzy_step failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

// All-pairs shortest paths: spx_apsp_plan / spx_apsp.
// Included from spx.hip after als_kernels.h.
//
// The blocked Floyd-Warshall recurrence over nb = ceil(n / TB) pivot blocks of
// edge TB = 64.  Everything is a (min, +) product of TB x TB tiles,
//
//   C[i][j] = min(C[i][j], min_k A[i][k] + B[k][j]),
//
// and only the diagonal tile has a dependence along k:
//
//   k_apsp_init   G -> D: 0 / +inf / the diagonal's own value become "no edge"
//                 (+inf), the diagonal 0, the undirected minimum of G and G^T;
//                 a negative or NaN entry stores -1 into *info (plain store);
//   per pivot block r:
//   k_apsp_diag   one workgroup closes tile (r, r): TB dependent pivot steps on
//                 a register micro-tile, row and column k + 1 republished in
//                 LDS after step k, one barrier a step;
//   k_apsp_panel  the 2 (nb - 1) tiles of block row r and block column r.  With
//                 the CLOSED diagonal tile T the dependent steps collapse into
//                 one product: X <- min(X, T (x) X) for a row tile, min(X, X (x) T)
//                 for a column tile (T holds every path inside the block, so the
//                 product over the original X is the closure; T's zero diagonal
//                 keeps X itself).  Each workgroup reads both operands whole
//                 before it stores, so updating X in place is safe;
//   k_apsp_rest   the (nb - 1)^2 other tiles, C <- min(C, D[i][r] (x) D[r][j]):
//                 the hot path, the same device function;
//   k_apsp_fill   rewrites +inf as `unreachable` when that is not +inf.
//
// The product (`minplus_tile`): 256 threads, a 4 x 4 micro-tile per lane.  LDS
// holds KC values of k at a time, A as [TB][KC + V] and B as [KC][TB] (V = 16
// bytes of elements; KC = TB in the panel launch, where one workgroup a CU runs
// and occupancy is not the limit, KC = KR = 16 in k_apsp_rest, where 9 / 17 KiB
// a workgroup leave the occupancy to the registers; DESIGN.md 3.23 has the
// reasoning).  Per V
// steps of k a lane reads 4 vectors A[i0 + r][k .. k + V) and V x (4 / V)
// vectors B[k][its columns], all 16-byte reads, for 16 V add+min pairs.  A lane
// is (ty, tx) = (tid / 16, tid % 16), rows 4 ty + r, columns
// (c / V) 16 V + tx V + c % V.  Bank rules (16-byte reads, groups of 16 lanes,
// bank = dword address mod 64): the A read is one address per ty (broadcast
// over tx) and the row pad puts the up to two ty of a lane group 16 banks
// apart; the B read of the 16 tx of a group is one contiguous 256-byte line.
// Both are conflict-free.
//
// Rows and columns past n are +inf in LDS and masked at the store; after init
// no -inf exists, so inf + x is never NaN.  No atomics, no host
// synchronisation; the same input gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

namespace spx_graph {

typedef int64_t i64;

constexpr int TB = 64;   // pivot-block edge, both dtypes
constexpr int NT = 256;  // threads of every tile kernel
constexpr int MT = 4;    // micro-tile edge
constexpr int KR = 16;   // k_apsp_rest stages its operands in chunks of KR values of k

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

template <typename T>
__device__ inline T vget(const typename Vec<T>::type& v, int i);
template <>
__device__ inline float vget<float>(const float4& v, int i) {
  return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}
template <>
__device__ inline double vget<double>(const double2& v, int i) {
  return i == 0 ? v.x : v.y;
}

template <typename T>
__device__ inline typename Vec<T>::type vmake(const T* p);
template <>
__device__ inline float4 vmake<float>(const float* p) {
  return make_float4(p[0], p[1], p[2], p[3]);
}
template <>
__device__ inline double2 vmake<double>(const double* p) {
  return make_double2(p[0], p[1]);
}

template <typename T>
__device__ inline T tmin(T a, T b);
template <>
__device__ inline float tmin<float>(float a, float b) {
  return __builtin_fminf(a, b);
}
template <>
__device__ inline double tmin<double>(double a, double b) {
  return __builtin_fmin(a, b);
}

template <typename T>
constexpr int lda_of() {
  return TB + Vec<T>::V;
}

// column c (0 .. 3) of lane tx's micro-tile
template <typename T>
__device__ inline int col_of(int tx, int c) {
  constexpr int V = Vec<T>::V;
  return (c / V) * (16 * V) + tx * V + (c % V);
}

// One TB x TB tile at (row0, col0) of D into LDS rows of stride `ld`; +inf
// outside the matrix.  16-byte global loads where `vec` (base and leading
// dimension 16-byte aligned) and the vector lies inside the row.
template <typename T, int ROWS = TB, int COLS = TB>
__device__ inline void stage_tile(T* __restrict__ dst, int ld, const T* __restrict__ D, i64 ldd, i64 n, i64 row0,
                                  i64 col0, bool vec, int tid) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::V;
  const T inf = std::numeric_limits<T>::infinity();
  constexpr int VPR = COLS / V;  // vectors per row
  static_assert((ROWS * VPR) % NT == 0, "the block is a whole number of vectors per thread");
#pragma unroll
  for (int it = 0; it < ROWS * VPR / NT; ++it) {
    const int idx = it * NT + tid;
    const int r = idx / VPR, cv = (idx % VPR) * V;
    const i64 gr = row0 + r, gc = col0 + cv;
    T* out = dst + r * ld + cv;
    if (gr < n && vec && gc + V <= n) {
      *(VT*)out = *(const VT*)(D + gr * ldd + gc);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) out[e] = (gr < n && gc + e < n) ? D[gr * ldd + gc + e] : inf;
    }
  }
}

// A lane's micro-tile from / to D: 16-byte accesses where `vec` and the vector
// lies inside the matrix, masked elements otherwise.
template <typename T>
__device__ inline void load_micro(T (&c)[MT][MT], const T* __restrict__ D, i64 ldd, i64 n, i64 row0, i64 col0, int ty,
                                  int tx, bool vec) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::V;
  const T inf = std::numeric_limits<T>::infinity();
#pragma unroll
  for (int r = 0; r < MT; ++r)
#pragma unroll
    for (int g = 0; g < MT / V; ++g) {
      const i64 gr = row0 + ty * MT + r, gc = col0 + col_of<T>(tx, g * V);
      if (gr < n && vec && gc + V <= n) {
        const VT v = *(const VT*)(D + gr * ldd + gc);
#pragma unroll
        for (int e = 0; e < V; ++e) c[r][g * V + e] = vget<T>(v, e);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) c[r][g * V + e] = (gr < n && gc + e < n) ? D[gr * ldd + gc + e] : inf;
      }
    }
}

template <typename T>
__device__ inline void store_micro(const T (&c)[MT][MT], T* __restrict__ D, i64 ldd, i64 n, i64 row0, i64 col0, int ty,
                                   int tx, bool vec) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::V;
#pragma unroll
  for (int r = 0; r < MT; ++r)
#pragma unroll
    for (int g = 0; g < MT / V; ++g) {
      const i64 gr = row0 + ty * MT + r, gc = col0 + col_of<T>(tx, g * V);
      if (gr < n && vec && gc + V <= n) {
        *(VT*)(D + gr * ldd + gc) = vmake<T>(&c[r][g * V]);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (gr < n && gc + e < n) D[gr * ldd + gc + e] = c[r][g * V + e];
      }
    }
}

// c = min(c, As (x) Bs) over KC values of k; As [TB][KC + V], Bs [KC][TB].
template <typename T, int KC = TB>
__device__ inline void minplus_tile(T (&c)[MT][MT], const T* __restrict__ As, const T* __restrict__ Bs, int ty,
                                    int tx) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::V, LDA = KC + V;
#pragma unroll 4
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
        for (int cc = 0; cc < MT; ++cc)
          c[r][cc] = tmin<T>(c[r][cc], vget<T>(a[r], kk) + vget<T>(b[cc / V], cc % V));
    }
  }
}

// The tile (ti, tj) <- min(itself, D[ti][r] (x) D[r][tj]), the operands staged
// in chunks of KC values of k (A as [TB][KC + V], B as [KC][TB]).  Every chunk
// is read from global memory before the one store at the end, so (ti, tj) may be
// one of the operands (the panel launch).
template <typename T, int KC = TB>
__device__ inline void update_tile(T* __restrict__ D, i64 ldd, i64 n, i64 r, i64 ti, i64 tj, bool vec) {
  constexpr int V = Vec<T>::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char graph_smem[];
  T* As = (T*)graph_smem;
  T* Bs = As + TB * (KC + V);
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  T c[MT][MT];
  load_micro<T>(c, D, ldd, n, ti * TB, tj * TB, ty, tx, vec);
#pragma unroll 1
  for (int kc = 0; kc < TB; kc += KC) {
    if (kc) __syncthreads();  // the chunk before has been read
    stage_tile<T, TB, KC>(As, KC + V, D, ldd, n, ti * TB, r * TB + kc, vec, tid);
    stage_tile<T, KC, TB>(Bs, TB, D, ldd, n, r * TB + kc, tj * TB, vec, tid);
    __syncthreads();
    minplus_tile<T, KC>(c, As, Bs, ty, tx);
  }
  store_micro<T>(c, D, ldd, n, ti * TB, tj * TB, ty, tx, vec);
}

template <typename T, int KC>
constexpr size_t lds_kc() {
  return (size_t)(TB * (KC + Vec<T>::V) + KC * TB) * sizeof(T);
}

template <typename T>
__global__ __launch_bounds__(NT) void k_apsp_rest(T* __restrict__ D, i64 ldd, i64 n, i64 r, int vec) {
  // grid (nb - 1, nb - 1): the tile indices skip the pivot block
  const i64 ti = blockIdx.y + (blockIdx.y >= r ? 1 : 0), tj = blockIdx.x + (blockIdx.x >= r ? 1 : 0);
  update_tile<T, KR>(D, ldd, n, r, ti, tj, vec != 0);
}

template <typename T>
__global__ __launch_bounds__(NT) void k_apsp_panel(T* __restrict__ D, i64 ldd, i64 n, i64 r, int vec) {
  // grid (nb - 1, 2): y = 0 the tiles of block row r, y = 1 those of block column r
  const i64 t = blockIdx.x + (blockIdx.x >= r ? 1 : 0);
  if (blockIdx.y == 0)
    update_tile<T>(D, ldd, n, r, r, t, vec != 0);
  else
    update_tile<T>(D, ldd, n, r, t, r, vec != 0);
}

// The closure of the diagonal tile r.  The micro-tiles stay in registers; LDS
// (stride lda_of) holds what the pivot steps read: row k and column k at step k.
// Step k changes neither (d[k][k] = 0 and no weight is negative), so the one
// barrier of a step separates the publication of row / column k + 1 from their
// use; the entries where they cross row / column k are rewritten with the bits
// they already hold.
template <typename T>
__global__ __launch_bounds__(NT) void k_apsp_diag(T* __restrict__ D, i64 ldd, i64 n, i64 r, int vec) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::V, LD = lda_of<T>();
  extern __shared__ __attribute__((aligned(16))) unsigned char graph_smem[];
  T* t = (T*)graph_smem;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const i64 o = r * TB;
  stage_tile<T>(t, LD, D, ldd, n, o, o, vec != 0, tid);
  T c[MT][MT];
  load_micro<T>(c, D, ldd, n, o, o, ty, tx, vec != 0);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TB; ++k) {
    T a[MT];
    VT b[MT / V];
#pragma unroll
    for (int rr = 0; rr < MT; ++rr) a[rr] = t[(ty * MT + rr) * LD + k];
#pragma unroll
    for (int g = 0; g < MT / V; ++g) b[g] = *(const VT*)(t + k * LD + g * (16 * V) + tx * V);
#pragma unroll
    for (int rr = 0; rr < MT; ++rr)
#pragma unroll
      for (int cc = 0; cc < MT; ++cc) c[rr][cc] = tmin<T>(c[rr][cc], a[rr] + vget<T>(b[cc / V], cc % V));
    if (k + 1 < TB) {
      const int q = k + 1;  // a constant of the unrolled step
      if (ty == q / MT) {
#pragma unroll
        for (int cc = 0; cc < MT; ++cc) t[q * LD + col_of<T>(tx, cc)] = c[q % MT][cc];
      }
      const int qc = (q / (16 * V)) * V + q % V;  // the micro-tile column that is matrix column q ...
      if (tx == (q % (16 * V)) / V) {             // ... in this lane
#pragma unroll
        for (int rr = 0; rr < MT; ++rr) t[(ty * MT + rr) * LD + q] = c[rr][qc];
      }
    }
    __syncthreads();
  }
  store_micro<T>(c, D, ldd, n, o, o, ty, tx, vec != 0);
}

// G -> D.  32 x 32 tiles; the undirected case reads the mirrored tile through
// LDS so that both reads of G are along rows.
template <typename T>
__global__ __launch_bounds__(NT) void k_apsp_init(int directed, i64 n, const T* __restrict__ G, i64 ldg,
                                                  T* __restrict__ D, i64 ldd, int32_t* __restrict__ info) {
  __shared__ T mir[32][33];
  const T inf = std::numeric_limits<T>::infinity();
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;  // 32 x 8
  const i64 r0 = (i64)blockIdx.y * 32, c0 = (i64)blockIdx.x * 32;
  bool bad = false;
  if (!directed) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const i64 gr = c0 + ly + 8 * s, gc = r0 + lx;  // the tile at (c0, r0)
      mir[ly + 8 * s][lx] = (gr < n && gc < n) ? G[gr * ldg + gc] : inf;
    }
    __syncthreads();
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int li = ly + 8 * s;
    const i64 gr = r0 + li, gc = c0 + lx;
    if (gr < n && gc < n) {
      const T g = G[gr * ldg + gc];
      bad = bad || !(g >= (T)0);  // negative, -inf or NaN
      T w = (g > (T)0 && g < inf) ? g : inf;
      if (!directed) {
        const T h = mir[lx][li];  // G[gc][gr]
        if (h > (T)0 && h < inf) w = tmin<T>(w, h);
      }
      D[gr * ldd + gc] = gr == gc ? (T)0 : w;
    }
  }
  if (bad) *info = -1;  // the same value from every thread that stores
}

template <typename T>
__global__ __launch_bounds__(NT) void k_apsp_fill(i64 n, T* __restrict__ D, i64 ldd, T value) {
  const i64 gc = (i64)blockIdx.x * NT + threadIdx.x;
  if (gc >= n) return;
  for (i64 gr = blockIdx.y; gr < n; gr += gridDim.y) {
    T* p = D + gr * ldd + gc;
    if (*p == std::numeric_limits<T>::infinity()) *p = value;
  }
}

template <typename T>
static hipError_t run(int directed, i64 n, const T* G, i64 ldg, T* D, i64 ldd, double unreachable, int32_t* info,
                      hipStream_t s) {
  hipError_t e = hipMemsetAsync(info, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  const unsigned g32 = (unsigned)((n + 31) / 32);
  hipLaunchKernelGGL((k_apsp_init<T>), dim3(g32, g32), dim3(NT), 0, s, directed, n, G, ldg, D, ldd, info);
  const i64 nb = (n + TB - 1) / TB;
  const int vec = ((uintptr_t)D % 16 == 0 && (ldd * sizeof(T)) % 16 == 0) ? 1 : 0;
  // each kernel asks for what it uses: the diagonal one tile (17 / 34 KiB), the
  // panel two whole tiles (33 / 66 KiB), the rest two chunks of KR (9 / 17 KiB)
  constexpr size_t lds_diag = (size_t)TB * lda_of<T>() * sizeof(T), lds_panel = lds_kc<T, TB>();
  static_assert(lds_diag <= 48 * 1024 && lds_kc<T, KR>() <= 48 * 1024, "only the panel may need the attribute");
  if (lds_panel > 48 * 1024) {  // float64 only; set per call, as the attribute belongs to the current device
    e = hipFuncSetAttribute((const void*)k_apsp_panel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_panel);
    if (e != hipSuccess) return e;
  }
  for (i64 r = 0; r < nb; ++r) {
    hipLaunchKernelGGL((k_apsp_diag<T>), dim3(1), dim3(NT), lds_diag, s, D, ldd, n, r, vec);
    if (nb > 1) {
      hipLaunchKernelGGL((k_apsp_panel<T>), dim3((unsigned)(nb - 1), 2), dim3(NT), lds_panel, s, D, ldd, n, r, vec);
      hipLaunchKernelGGL((k_apsp_rest<T>), dim3((unsigned)(nb - 1), (unsigned)(nb - 1)), dim3(NT), (lds_kc<T, KR>()),
                         s, D, ldd, n, r, vec);
    }
  }
  if (!(unreachable == std::numeric_limits<double>::infinity()))
    hipLaunchKernelGGL((k_apsp_fill<T>), dim3((unsigned)((n + NT - 1) / NT), (unsigned)(n < 65535 ? n : 65535)),
                       dim3(NT), 0, s, n, D, ldd, (T)unreachable);
  return hipGetLastError();
}

}  // namespace spx_graph

// ------------------------------------------------------------------ C ABI
extern "C" int spx_apsp_plan(int dtype, int64_t* tile) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_apsp_plan: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_apsp_plan: dtype %d is not float32 / float64", dtype);
  if (tile) *tile = spx_graph::TB;
  return SPX_OK;
}

extern "C" int spx_apsp(int dtype, int directed, int64_t n, const void* G, int64_t ldg, void* D, int64_t ldd,
                        double unreachable, int32_t* info, void* stream) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_apsp: bad dtype %d", dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "spx_apsp: dtype %d is not float32 / float64", dtype);
  if (n < 0) return set_err(SPX_EINVAL, "spx_apsp: negative size (n %lld)", (long long)n);
  if (!(unreachable >= 0.0))
    return set_err(SPX_EINVAL, "spx_apsp: unreachable = %g is negative or NaN", unreachable);
  if (n == 0) return SPX_OK;
  if (!G || !D || !info) return set_err(SPX_EINVAL, "spx_apsp: null pointer");
  if (ldg < n || ldd < n)
    return set_err(SPX_EINVAL, "spx_apsp: leading dimension (ldg %lld, ldd %lld) below n = %lld", (long long)ldg,
                   (long long)ldd, (long long)n);
  if (D == G) return set_err(SPX_EINVAL, "spx_apsp: D may not be G (the first pass reads G[j][i] while it writes D)");
  if (n > 65535LL * 32)
    return set_err(SPX_ENOTSUP, "spx_apsp: n = %lld is above the limit %lld", (long long)n, 65535LL * 32);
  hipError_t e = dtype == SPX_F32 ? spx_graph::run<float>(directed != 0, n, (const float*)G, ldg, (float*)D, ldd,
                                                          unreachable, info, S(stream))
                                  : spx_graph::run<double>(directed != 0, n, (const double*)G, ldg, (double*)D, ldd,
                                                           unreachable, info, S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_apsp failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

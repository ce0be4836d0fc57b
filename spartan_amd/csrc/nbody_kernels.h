// Direct-sum gravitational accelerations (spx_nbody_accel / spx_nbody_plan,
// include/spx.h): for every target j
//
//   a_j = sum_i G m_i (p_i - p_j) / r_ij^3,   r_ij = max(|p_i - p_j|, rmin),
//
// the reference's spartan/examples/nbody.py move() without its (n, n) arrays.
//
// k_nbody: a workgroup of NT lanes owns NT * TPL targets (TPL per lane, held
// in registers, consecutive lanes on consecutive targets) and one contiguous
// range of sources (blockIdx.y of `splits`).  It stages TS sources at a time
// in LDS as (x, y, z, G m) records; every lane then sweeps the tile.  The
// source index is wave-uniform, so a record is one broadcast ds_read_b128
// (two in float64) serving TPL interactions.  Per interaction: three
// differences, r^2, the clamp as a compare and select on r^2 (false for NaN,
// so NaN goes through), ONE reciprocal square root, and
// ((G m) inv_r) inv_r) inv_r) d -- r^3 is never formed, so float32 data on
// the reference's scale (G m 1e20, r 1e14) stays in range.  The term of a
// pair at distance 0 is (G m / rmin^3) * 0 = 0 exactly: no index compare.
//
// float64: v_rsq_f64 (about 2^-23) and two Newton steps.  float32: v_rsq_f32.
// Sums: CH sources in T, then added to a float64 accumulator per target and
// component, so no float32 sum is longer than CH terms.  With splits == 1 the
// accumulators are stored as T; otherwise as float64 partials [split][3][n_tgt]
// that k_nbody_sum adds in ascending split order.  No atomics.
//
// SPX_NBODY_SCALAR_SRC=1 builds the alternative that was measured against the
// LDS tile: no staging, the uniform source index read
// straight from global memory (scalar loads).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#ifndef SPX_NBODY_SCALAR_SRC
#define SPX_NBODY_SCALAR_SRC 0
#endif
#ifndef SPX_NBODY_TPL  // (1 and 2 were measured against 4: DESIGN.md 3.26)
#define SPX_NBODY_TPL 4
#endif

namespace spx_nbody {

typedef int64_t i64;

constexpr int NT = 256;          // lanes of a workgroup
constexpr int TPL = SPX_NBODY_TPL;  // targets per lane
constexpr int TPB = NT * TPL;    // targets per workgroup
constexpr int TS = 512;          // sources per LDS tile
constexpr int CH = 32;           // sources per partial sum in T
constexpr int RANGE_MIN = 128;   // the planner's shortest source range
constexpr i64 SPLITS_MAX = 1024; // source ranges (grid.y)
static_assert(TS % NT == 0 && TS % CH == 0, "whole staging passes and whole chunks per tile");

template <typename T>
struct alignas(16) Src {
  T x, y, z, gm;
};

__device__ __forceinline__ float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ double rsq(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double h = 0.5 * x;
#pragma unroll
  for (int it = 0; it < 2; ++it) y = __builtin_fma(y, __builtin_fma(-(h * y), y, 0.5), y);
  return y;
}
__device__ __forceinline__ float fmad(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fmad(double a, double b, double c) { return __builtin_fma(a, b, c); }

// one source against the lane's TPL targets
template <typename T>
__device__ __forceinline__ void interact(T sx, T sy, T sz, T gm, T rmin2, const T (&tx)[TPL], const T (&ty)[TPL],
                                         const T (&tz)[TPL], T (&px)[TPL], T (&py)[TPL], T (&pz)[TPL]) {
#pragma unroll
  for (int k = 0; k < TPL; ++k) {
    const T dx = sx - tx[k], dy = sy - ty[k], dz = sz - tz[k];
    const T r2 = fmad(dz, dz, fmad(dy, dy, dx * dx));
    const T inv = rsq(r2 < rmin2 ? rmin2 : r2);
    const T w = ((gm * inv) * inv) * inv;
    px[k] = fmad(w, dx, px[k]);
    py[k] = fmad(w, dy, py[k]);
    pz[k] = fmad(w, dz, pz[k]);
  }
}

template <typename T, bool SCALAR>
__global__ __launch_bounds__(NT) void k_nbody(i64 n_tgt, const T* __restrict__ tgx, const T* __restrict__ tgy,
                                              const T* __restrict__ tgz, i64 n_src, i64 per_split,
                                              const T* __restrict__ sx, const T* __restrict__ sy,
                                              const T* __restrict__ sz, const T* __restrict__ sm, double G, T rmin2,
                                              T* __restrict__ ax, T* __restrict__ ay, T* __restrict__ az,
                                              double* __restrict__ part) {
  __shared__ Src<T> tile[SCALAR ? 1 : TS];
  const int tid = (int)threadIdx.x;
  const i64 t0 = (i64)blockIdx.x * TPB + tid;
  const i64 sbeg = (i64)blockIdx.y * per_split;
  const i64 send = sbeg + per_split < n_src ? sbeg + per_split : n_src;  // (may be <= sbeg: an empty range)

  T tx[TPL], ty[TPL], tz[TPL];
  double accx[TPL], accy[TPL], accz[TPL];
#pragma unroll
  for (int k = 0; k < TPL; ++k) {
    const i64 t = t0 + (i64)k * NT;
    const bool in = t < n_tgt;
    tx[k] = in ? tgx[t] : (T)0;
    ty[k] = in ? tgy[t] : (T)0;
    tz[k] = in ? tgz[t] : (T)0;
    accx[k] = accy[k] = accz[k] = 0.0;
  }

  if (SCALAR) {
#pragma unroll 1
    for (i64 j0 = sbeg; j0 < send; j0 += CH) {
      const i64 j1 = j0 + CH < send ? j0 + CH : send;
      T px[TPL] = {}, py[TPL] = {}, pz[TPL] = {};
#pragma unroll 4
      for (i64 j = j0; j < j1; ++j) interact<T>(sx[j], sy[j], sz[j], (T)(G * (double)sm[j]), rmin2, tx, ty, tz, px, py, pz);
#pragma unroll
      for (int k = 0; k < TPL; ++k) {
        accx[k] += (double)px[k];
        accy[k] += (double)py[k];
        accz[k] += (double)pz[k];
      }
    }
  } else {
#pragma unroll 1
    for (i64 s0 = sbeg; s0 < send; s0 += TS) {
      const int cnt = (int)(send - s0 < TS ? send - s0 : TS);
      __syncthreads();  // the previous tile has been read by every wave
#pragma unroll
      for (int i = tid; i < TS; i += NT)
        if (i < cnt) {
          Src<T> r;
          r.x = sx[s0 + i];
          r.y = sy[s0 + i];
          r.z = sz[s0 + i];
          r.gm = (T)(G * (double)sm[s0 + i]);
          tile[i] = r;
        }
      __syncthreads();
#pragma unroll 1
      for (int j0 = 0; j0 < cnt; j0 += CH) {
        const int j1 = j0 + CH < cnt ? j0 + CH : cnt;
        T px[TPL] = {}, py[TPL] = {}, pz[TPL] = {};
        if (j1 - j0 == CH) {
#pragma unroll 8
          for (int j = 0; j < CH; ++j) {
            const Src<T> r = tile[j0 + j];
            interact<T>(r.x, r.y, r.z, r.gm, rmin2, tx, ty, tz, px, py, pz);
          }
        } else {
#pragma unroll 1
          for (int j = j0; j < j1; ++j) {
            const Src<T> r = tile[j];
            interact<T>(r.x, r.y, r.z, r.gm, rmin2, tx, ty, tz, px, py, pz);
          }
        }
#pragma unroll
        for (int k = 0; k < TPL; ++k) {
          accx[k] += (double)px[k];
          accy[k] += (double)py[k];
          accz[k] += (double)pz[k];
        }
      }
    }
  }

#pragma unroll
  for (int k = 0; k < TPL; ++k) {
    const i64 t = t0 + (i64)k * NT;
    if (t < n_tgt) {
      if (part) {  // [split][component][target]
        double* p = part + (i64)blockIdx.y * 3 * n_tgt + t;
        p[0] = accx[k];
        p[n_tgt] = accy[k];
        p[2 * n_tgt] = accz[k];
      } else {
        ax[t] = (T)accx[k];
        ay[t] = (T)accy[k];
        az[t] = (T)accz[k];
      }
    }
  }
}

// out[c][t] = sum over the splits, in ascending order, of part[s][c][t]
template <typename T>
__global__ __launch_bounds__(NT) void k_nbody_sum(i64 n_tgt, i64 splits, const double* __restrict__ part,
                                                  T* __restrict__ ax, T* __restrict__ ay, T* __restrict__ az) {
  const i64 t = (i64)blockIdx.x * NT + threadIdx.x;
  if (t >= n_tgt) return;
  double a[3] = {0.0, 0.0, 0.0};
  for (i64 s = 0; s < splits; ++s)
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] += part[(s * 3 + c) * n_tgt + t];
  ax[t] = (T)a[0];
  ay[t] = (T)a[1];
  az[t] = (T)a[2];
}

// ------------------------------------------------------------------- plan
// The source ranges: enough workgroups for two per CU, no range shorter than
// RANGE_MIN sources, never more than SPLITS_MAX.  Pure arithmetic.
static i64 plan_splits(i64 n_tgt, i64 n_src, i64 cus) {
  if (n_tgt < 1 || n_src < 1) return 1;
  const i64 blocks = (n_tgt + TPB - 1) / TPB, most = (n_src + RANGE_MIN - 1) / RANGE_MIN;
  i64 s = (2 * cus + blocks - 1) / blocks;
  if (s > most) s = most;
  if (s > SPLITS_MAX) s = SPLITS_MAX;
  return s < 1 ? 1 : s;
}

static i64 workspace_for(i64 n_tgt, i64 splits) { return splits > 1 ? splits * 3 * n_tgt * 8 : 0; }

template <typename T>
static hipError_t run(i64 n_tgt, const T* tx, const T* ty, const T* tz, i64 n_src, const T* sx, const T* sy,
                      const T* sz, const T* sm, double G, double rmin, T* ax, T* ay, T* az, i64 splits, double* part,
                      hipStream_t s) {
  const i64 blocks = (n_tgt + TPB - 1) / TPB;
  const i64 per = (n_src + splits - 1) / splits;  // (the trailing ranges of a forced split may be empty: zeros)
  k_nbody<T, SPX_NBODY_SCALAR_SRC != 0><<<dim3((unsigned)blocks, (unsigned)splits), NT, 0, s>>>(
      n_tgt, tx, ty, tz, n_src, per, sx, sy, sz, sm, G, (T)(rmin * rmin), ax, ay, az, splits > 1 ? part : nullptr);
  if (splits > 1) k_nbody_sum<T><<<(unsigned)((n_tgt + NT - 1) / NT), NT, 0, s>>>(n_tgt, splits, part, ax, ay, az);
  return hipGetLastError();
}

}  // namespace spx_nbody

// ------------------------------------------------------------------ C ABI
static int nbody_check(const char* who, int dtype, int64_t n_tgt, int64_t n_src, int64_t splits) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "%s: bad dtype %d", who, dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "%s: dtype %d is not float32 / float64", who, dtype);
  if (n_tgt < 0 || n_src < 0)
    return set_err(SPX_EINVAL, "%s: negative size (n_tgt %lld, n_src %lld)", who, (long long)n_tgt, (long long)n_src);
  if (n_tgt > (int64_t)spx_nbody::TPB * 0x7fffffffLL)
    return set_err(SPX_ENOTSUP, "%s: n_tgt = %lld is above the grid limit", who, (long long)n_tgt);
  if (n_src > (1LL << 48))
    return set_err(SPX_ENOTSUP, "%s: n_src = %lld is above the limit 2^48", who, (long long)n_src);
  if (splits < 0 || splits > spx_nbody::SPLITS_MAX)
    return set_err(SPX_EINVAL, "%s: splits = %lld is outside 0 .. %lld", who, (long long)splits,
                   (long long)spx_nbody::SPLITS_MAX);
  return SPX_OK;
}

extern "C" int spx_nbody_plan(int dtype, int64_t n_tgt, int64_t n_src, int64_t* tgt_per_block, int64_t* splits,
                              size_t* workspace_bytes) {
  if (tgt_per_block) *tgt_per_block = spx_nbody::TPB;
  const int64_t forced = splits ? *splits : 0;
  int rc = nbody_check("spx_nbody_plan", dtype, n_tgt, n_src, forced);
  if (rc != SPX_OK) return rc;
  const int64_t use = forced > 0 ? forced : spx_nbody::plan_splits(n_tgt, n_src, num_cus());
  if (splits) *splits = use;
  if (workspace_bytes) *workspace_bytes = (size_t)spx_nbody::workspace_for(n_tgt, use);
  return SPX_OK;
}

extern "C" int spx_nbody_accel(int dtype, int64_t n_tgt, const void* tx, const void* ty, const void* tz,
                               int64_t n_src, const void* sx, const void* sy, const void* sz, const void* sm, double G,
                               double rmin, void* ax, void* ay, void* az, int64_t splits, void* workspace,
                               size_t workspace_bytes, void* stream) {
  int rc = nbody_check("spx_nbody_accel", dtype, n_tgt, n_src, splits);
  if (rc != SPX_OK) return rc;
  if (!std::isfinite(G)) return set_err(SPX_EINVAL, "spx_nbody_accel: G = %g is not finite", G);
  if (!(rmin >= 0.0) || !std::isfinite(rmin))
    return set_err(SPX_EINVAL, "spx_nbody_accel: rmin = %g is not finite and >= 0", rmin);
  if (n_tgt == 0) return SPX_OK;
  if (!tx || !ty || !tz || !ax || !ay || !az) return set_err(SPX_EINVAL, "spx_nbody_accel: null pointer (targets / outputs)");
  const size_t esz = dtype == SPX_F32 ? 4 : 8;
  if (n_src == 0) {
    HIP_TRY(hipMemsetAsync(ax, 0, (size_t)n_tgt * esz, S(stream)));
    HIP_TRY(hipMemsetAsync(ay, 0, (size_t)n_tgt * esz, S(stream)));
    HIP_TRY(hipMemsetAsync(az, 0, (size_t)n_tgt * esz, S(stream)));
    return SPX_OK;
  }
  if (!sx || !sy || !sz || !sm) return set_err(SPX_EINVAL, "spx_nbody_accel: null pointer (sources)");
  const int64_t use = splits > 0 ? splits : spx_nbody::plan_splits(n_tgt, n_src, num_cus());
  const int64_t need = spx_nbody::workspace_for(n_tgt, use);
  if (need > 0) {
    if (!workspace || (int64_t)workspace_bytes < need)
      return set_err(SPX_EINVAL, "spx_nbody_accel: workspace %zu < %lld bytes for %lld splits", workspace_bytes,
                     (long long)need, (long long)use);
    if ((uintptr_t)workspace % 8 != 0) return set_err(SPX_EINVAL, "spx_nbody_accel: workspace is not 8-byte aligned");
  }
  hipError_t e = dtype == SPX_F32
                     ? spx_nbody::run<float>(n_tgt, (const float*)tx, (const float*)ty, (const float*)tz, n_src,
                                             (const float*)sx, (const float*)sy, (const float*)sz, (const float*)sm, G,
                                             rmin, (float*)ax, (float*)ay, (float*)az, use, (double*)workspace,
                                             S(stream))
                     : spx_nbody::run<double>(n_tgt, (const double*)tx, (const double*)ty, (const double*)tz, n_src,
                                              (const double*)sx, (const double*)sy, (const double*)sz,
                                              (const double*)sm, G, rmin, (double*)ax, (double*)ay, (double*)az, use,
                                              (double*)workspace, S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_nbody_accel failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

// Prefix-sum (np.cumsum) kernels behind spx_scan / spx_scan_workspace
// (include/spx.h).  Included from spx.hip after the error helpers.
//
// The input is a dense row-major block viewed as (outer, n, inner); the scan
// runs along n for each of the outer * inner lines.  Accumulation is unsigned
// 64-bit for bool / int32 / int64 inputs (wrap-around defined, result int64)
// and fp64 for both float types (an fp32 result is rounded once, on store).
//
// Two kernels, one per memory layout (each with a cheaper totals-only twin
// for out == NULL):
//   k_scan_row  (inner == 1): a line is contiguous.  A lane loads 4
//     consecutive elements per step (one vector load where the pointers and n
//     allow it, guarded scalar loads otherwise), scans them serially, the 64
//     lane sums are scanned across the wave with DPP moves, and -- when a
//     whole workgroup owns the line -- the four wave sums meet in LDS.  Short
//     lines get one wave each (no LDS, no barrier).
//   k_scan_col  (inner > 1): lanes run along inner (coalesced rows of 64
//     columns), each wave holds SCAN_RW rows in registers and the SCAN_CW
//     waves of a workgroup stack their row groups through LDS.
// Both walk their rows segment by segment with the carry in registers, so a
// line is read once ("line" mode).  When the lines are too few to fill the
// machine and long, the host cuts them into chunks of SCAN_CHUNK elements and
// runs three launches ("chunked" mode): chunk totals into the workspace, an
// exclusive scan of those totals in place (the same kernels, line mode), and
// the chunk scans with their bases -- the input is read twice.  No workgroup
// ever waits for another inside a launch: forward progress between
// workgroups is not guaranteed, so there is no look-back and no spin on
// global memory.  The addition order depends only on the geometry, and there
// are no atomics: same input, same geometry, same bits.

#define SCAN_CHUNK 32768  // elements of a line per chunk (chunked mode); a multiple of 4
#define SCAN_RW 16        // rows per wave and segment of k_scan_col

template <typename T> struct ScanT;
template <> struct ScanT<uint8_t> { typedef u64 A; typedef i64 O; };
template <> struct ScanT<int32_t> { typedef u64 A; typedef i64 O; };
template <> struct ScanT<int64_t> { typedef u64 A; typedef i64 O; };
template <> struct ScanT<float> { typedef double A; typedef float O; };
template <> struct ScanT<double> { typedef double A; typedef double O; };

__device__ __forceinline__ u64 scan_widen(uint8_t v) { return v ? 1ULL : 0ULL; }
__device__ __forceinline__ u64 scan_widen(int32_t v) { return (u64)(i64)v; }
__device__ __forceinline__ u64 scan_widen(int64_t v) { return (u64)v; }
__device__ __forceinline__ double scan_widen(float v) { return (double)v; }
__device__ __forceinline__ double scan_widen(double v) { return v; }

template <typename T>
using scan_v4 = T __attribute__((ext_vector_type(4)));

template <typename T>
struct ScanArgs {
  typedef typename ScanT<T>::A A;
  typedef typename ScanT<T>::O O;
  const T* in;
  O* out;          // NULL: totals only
  const A* carry;  // (outer, inner) added to every element of its line, or NULL
  const A* base;   // (outer, nc, inner) per-chunk bases, or NULL
  A* tot;          // (outer, nc, inner) each chunk's own inclusive total, or NULL
  i64 outer, n, inner;
  i64 nc, chunk;   // chunks per line and rows per chunk (nc == 1: chunk == n)
  int exclusive;
  int vec;         // k_scan_row: 4-element vector loads and stores are aligned
};

// One 32-bit half of a value through a DPP move; lanes the control gives no
// source (row edges, rows outside ROW_MASK) read 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int scan_dpp32(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false);
}
template <int CTRL, int ROW_MASK, typename A>
__device__ __forceinline__ A scan_dpp(A v) {
  static_assert(sizeof(A) == 8, "64-bit accumulators");
  int w[2];
  __builtin_memcpy(w, &v, 8);
  w[0] = scan_dpp32<CTRL, ROW_MASK>(w[0]);
  w[1] = scan_dpp32<CTRL, ROW_MASK>(w[1]);
  __builtin_memcpy(&v, w, 8);
  return v;
}

// Inclusive scan of one value per lane over the wave, in a fixed order:
// Hillis-Steele inside each row of 16 lanes (row_shr 1, 2, 4, 8, zero fill),
// then lane 15 of rows 0 / 2 into rows 1 / 3 (row_bcast:15) and lane 31 into
// rows 2 and 3 (row_bcast:31) -- DPP moves, no LDS traffic.
template <typename A>
__device__ __forceinline__ A scan_wave_incl(A v) {
  v += scan_dpp<0x111, 0xF>(v);
  v += scan_dpp<0x112, 0xF>(v);
  v += scan_dpp<0x114, 0xF>(v);
  v += scan_dpp<0x118, 0xF>(v);
  v += scan_dpp<0x142, 0xA>(v);
  v += scan_dpp<0x143, 0xC>(v);
  return v;
}

// 4 consecutive elements of a line at i, widened; past r1 they read 0
template <typename T>
__device__ __forceinline__ void scan_load4(const T* src, i64 i, i64 r1, int vec, typename ScanT<T>::A (&x)[4]) {
  typedef typename ScanT<T>::A A;
  if (vec && i + 4 <= r1) {
    const scan_v4<T> v = __builtin_nontemporal_load((const scan_v4<T>*)(src + i));
    x[0] = scan_widen(v.x);
    x[1] = scan_widen(v.y);
    x[2] = scan_widen(v.z);
    x[3] = scan_widen(v.w);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = i + k < r1 ? scan_widen(src[i + k]) : (A)0;
  }
}

// BLOCK: the four waves of a workgroup share one work item (a line or a chunk
// of it); else each wave takes its own item.
template <typename T, bool BLOCK>
__global__ __launch_bounds__(256) void k_scan_row(ScanArgs<T> a) {
  typedef typename ScanT<T>::A A;
  typedef typename ScanT<T>::O O;
  constexpr int U = sizeof(T) == 8 ? 2 : 4;  // vectors per lane and segment
  constexpr i64 WSEG = 64 * 4 * U;           // elements per wave and segment
  constexpr i64 SEG = BLOCK ? 4 * WSEG : WSEG;
  __shared__ A wtot[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i64 items = a.outer * a.nc;
  const i64 first = BLOCK ? (i64)blockIdx.x : (i64)blockIdx.x * 4 + wave;
  const i64 step = BLOCK ? (i64)gridDim.x : (i64)gridDim.x * 4;
  int buf = 0;
  for (i64 item = first; item < items; item += step) {
    const i64 o = item / a.nc, c = item - o * a.nc;
    const i64 r0 = c * a.chunk;
    const i64 r1 = r0 + a.chunk < a.n ? r0 + a.chunk : a.n;
    const T* src = a.in + o * a.n;
    O* dst = a.out + o * a.n;
    A base = 0;
    if (a.carry) base = a.carry[o];
    if (a.base) base += a.base[item];
    A run = 0;  // sum of the segments walked so far (without the base)
    for (i64 s = r0; s < r1; s += SEG) {
      const i64 w0 = s + (BLOCK ? wave * WSEG : 0);
      A x[U][4];
#pragma unroll
      for (int u = 0; u < U; ++u) scan_load4(src, w0 + ((i64)u * 64 + lane) * 4, r1, a.vec, x[u]);
      A lex[U];  // sum of everything before this lane's vector within the wave's part
      A wrun = 0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x[u][1] += x[u][0];
        x[u][2] += x[u][1];
        x[u][3] += x[u][2];
        const A inc = scan_wave_incl(x[u][3]);
        A ex = __shfl_up(inc, 1, 64);
        if (lane == 0) ex = 0;
        lex[u] = wrun + ex;
        wrun += __shfl(inc, 63, 64);
      }
      A woff = 0, stot = wrun;
      if (BLOCK) {
        if (lane == 0) wtot[buf][wave] = wrun;
        __syncthreads();
        stot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const A t = wtot[buf][w];
          if (w < wave) woff += t;
          stot += t;
        }
        buf ^= 1;  // the next segment writes the other half: one barrier per segment
      }
      const A off = (base + run) + woff;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const i64 i = w0 + ((i64)u * 64 + lane) * 4;
        const A lo = off + lex[u];
        O y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          y[k] = (O)(a.exclusive ? (k ? lo + x[u][k ? k - 1 : 0] : lo) : lo + x[u][k]);
        if (a.vec && i + 4 <= r1) {
          scan_v4<O> v;
          v.x = y[0];
          v.y = y[1];
          v.z = y[2];
          v.w = y[3];
          *(scan_v4<O>*)(dst + i) = v;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (i + k < r1) dst[i + k] = y[k];
        }
      }
      run += stot;
    }
    if (a.tot && lane == 0 && (!BLOCK || wave == 0)) a.tot[item] = run;
  }
}

// The totals-only pass of the same items (out == NULL): every lane sums its
// own vectors over the whole item, one wave scan and one LDS exchange per
// item.  (A fixed order of its own: a line's total may differ from the last
// element of its scan in the last fp64 bits; integers are exact.)
template <typename T, bool BLOCK>
__global__ __launch_bounds__(256) void k_scan_row_totals(ScanArgs<T> a) {
  typedef typename ScanT<T>::A A;
  constexpr int U = sizeof(T) == 8 ? 4 : 8;
  constexpr i64 WSEG = 64 * 4 * U;
  constexpr i64 SEG = BLOCK ? 4 * WSEG : WSEG;
  __shared__ A wtot[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i64 items = a.outer * a.nc;
  const i64 first = BLOCK ? (i64)blockIdx.x : (i64)blockIdx.x * 4 + wave;
  const i64 step = BLOCK ? (i64)gridDim.x : (i64)gridDim.x * 4;
  int buf = 0;
  for (i64 item = first; item < items; item += step) {
    const i64 o = item / a.nc, c = item - o * a.nc;
    const i64 r0 = c * a.chunk;
    const i64 r1 = r0 + a.chunk < a.n ? r0 + a.chunk : a.n;
    const T* src = a.in + o * a.n;
    A acc = 0;
    for (i64 s = r0 + (BLOCK ? wave * WSEG : 0); s < r1; s += SEG) {
      A x[U][4];
#pragma unroll
      for (int u = 0; u < U; ++u) scan_load4(src, s + ((i64)u * 64 + lane) * 4, r1, a.vec, x[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) acc += (x[u][0] + x[u][1]) + (x[u][2] + x[u][3]);
    }
    A run = __shfl(scan_wave_incl(acc), 63, 64);
    if (BLOCK) {
      if (lane == 0) wtot[buf][wave] = run;
      __syncthreads();
      run = ((wtot[buf][0] + wtot[buf][1]) + wtot[buf][2]) + wtot[buf][3];
      buf ^= 1;  // the next item writes the other half: one barrier per item
    }
    if (lane == 0 && (!BLOCK || wave == 0)) a.tot[item] = run;
  }
}

// One workgroup of SCAN_CW waves per (outer, chunk, 64-column block): wave w
// of a segment of SCAN_CW * SCAN_RW rows takes rows [w * SCAN_RW, (w + 1) *
// SCAN_RW).  The rows stay in registers in the input type: summed once for
// the wave's total, and again from the wave's base for the stores.  Row
// addresses are wave-uniform (scalar registers) plus the lane's column.
#define SCAN_CW 8
template <typename T>
__global__ __launch_bounds__(64 * SCAN_CW) void k_scan_col(ScanArgs<T> a) {
  typedef typename ScanT<T>::A A;
  typedef typename ScanT<T>::O O;
  __shared__ A wtot[2][SCAN_CW][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 ncb = (a.inner + 63) / 64;
  const i64 items = a.outer * a.nc * ncb;
  int buf = 0;
  for (i64 item = blockIdx.x; item < items; item += gridDim.x) {
    const i64 cb = item % ncb, t = item / ncb;
    const i64 c = t % a.nc, o = t / a.nc;
    const i64 col0 = cb * 64, col = col0 + lane;
    const bool act = col < a.inner;
    const i64 r0 = c * a.chunk;
    const i64 r1 = r0 + a.chunk < a.n ? r0 + a.chunk : a.n;
    const T* src = a.in + o * a.n * a.inner + col0;  // wave-uniform
    O* dst = a.out + o * a.n * a.inner + col0;
    A base = 0;
    if (act && a.carry) base = a.carry[o * a.inner + col];
    if (act && a.base) base += a.base[(o * a.nc + c) * a.inner + col];
    A run = 0;
    for (i64 s = r0; s < r1; s += SCAN_CW * SCAN_RW) {
      const i64 w0 = s + wave * SCAN_RW;
      T x[SCAN_RW];
#pragma unroll
      for (int k = 0; k < SCAN_RW; ++k)
        x[k] = (act && w0 + k < r1) ? __builtin_nontemporal_load(src + (w0 + k) * a.inner + lane) : (T)0;
      A wsum = 0;
#pragma unroll
      for (int k = 0; k < SCAN_RW; ++k) wsum += scan_widen(x[k]);
      wtot[buf][wave][lane] = wsum;
      __syncthreads();
      A woff = 0, stot = 0;
#pragma unroll
      for (int w = 0; w < SCAN_CW; ++w) {
        const A tw = wtot[buf][w][lane];
        if (w < wave) woff += tw;
        stot += tw;
      }
      buf ^= 1;  // the next segment writes the other half: one barrier per segment
      if (act) {
        A r = (base + run) + woff;
#pragma unroll
        for (int k = 0; k < SCAN_RW; ++k) {
          const A before = r;
          r += scan_widen(x[k]);
          if (w0 + k < r1) dst[(w0 + k) * a.inner + lane] = (O)(a.exclusive ? before : r);
        }
      }
      run += stot;
    }
    if (a.tot && act && wave == 0) a.tot[(o * a.nc + c) * a.inner + col] = run;
  }
}

// totals-only pass of the same items: no barrier inside the row walk
template <typename T>
__global__ __launch_bounds__(64 * SCAN_CW) void k_scan_col_totals(ScanArgs<T> a) {
  typedef typename ScanT<T>::A A;
  __shared__ A wtot[2][SCAN_CW][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 ncb = (a.inner + 63) / 64;
  const i64 items = a.outer * a.nc * ncb;
  int buf = 0;
  for (i64 item = blockIdx.x; item < items; item += gridDim.x) {
    const i64 cb = item % ncb, t = item / ncb;
    const i64 c = t % a.nc, o = t / a.nc;
    const i64 col0 = cb * 64, col = col0 + lane;
    const bool act = col < a.inner;
    const i64 r0 = c * a.chunk;
    const i64 r1 = r0 + a.chunk < a.n ? r0 + a.chunk : a.n;
    const T* src = a.in + o * a.n * a.inner + col0;  // wave-uniform
    A acc = 0;
    for (i64 w0 = r0 + wave * SCAN_RW; w0 < r1; w0 += SCAN_CW * SCAN_RW) {
      T x[SCAN_RW];
#pragma unroll
      for (int k = 0; k < SCAN_RW; ++k)
        x[k] = (act && w0 + k < r1) ? __builtin_nontemporal_load(src + (w0 + k) * a.inner + lane) : (T)0;
#pragma unroll
      for (int k = 0; k < SCAN_RW; ++k) acc += scan_widen(x[k]);
    }
    wtot[buf][wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && act) {
      A run = 0;
#pragma unroll
      for (int w = 0; w < SCAN_CW; ++w) run += wtot[buf][w][lane];
      a.tot[(o * a.nc + c) * a.inner + col] = run;
    }
    buf ^= 1;  // the next item writes the other half: one barrier per item
  }
}

// ------------------------------------------------------------------ host
static int scan_num_cus() {
  static int ncu = 0;
  if (ncu == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      ncu = v;
    else
      ncu = 256;  // no device (argument checks, workspace queries): the MI355X's count
  }
  return ncu;
}

// chunked mode: long lines, and fewer independent work items in line mode
// than two per CU
static bool scan_chunked(i64 outer, i64 n, i64 inner) {
  if (n <= SCAN_CHUNK) return false;
  const i64 par = inner == 1 ? outer : outer * ((inner + 63) / 64);
  return par < 2 * (i64)scan_num_cus();
}

static bool scan_geom_ok(i64 outer, i64 n, i64 inner) {
  if (outer < 1 || n < 1 || inner < 1) return false;
  const i64 lim = (i64)1 << 60;
  if (outer > lim / n) return false;
  return outer * n <= lim / inner;
}

static bool scan_aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

// one launch: (outer, n, inner) cut into nc chunks of `chunk` rows
template <typename T>
static int scan_launch(const void* in, void* out, i64 outer, i64 n, i64 inner, i64 nc, i64 chunk,
                       const void* carry, const void* base, void* tot, int exclusive, hipStream_t st) {
  typedef typename ScanT<T>::A A;
  typedef typename ScanT<T>::O O;
  ScanArgs<T> a;
  a.in = (const T*)in;
  a.out = (O*)out;
  a.carry = (const A*)carry;
  a.base = (const A*)base;
  a.tot = (A*)tot;
  a.outer = outer;
  a.n = n;
  a.inner = inner;
  a.nc = nc;
  a.chunk = chunk;
  a.exclusive = exclusive ? 1 : 0;
  a.vec = 0;
  const i64 cap = (i64)1 << 20;
  if (inner == 1) {
    const i64 items = outer * nc;
    a.vec = scan_aligned(in, 4 * sizeof(T)) && (!out || scan_aligned(out, 4 * sizeof(O))) &&
            (n % 4 == 0 || outer == 1) && (chunk % 4 == 0 || nc == 1);
    const i64 g1 = items < cap ? items : cap, g4 = (items + 3) / 4 < cap ? (items + 3) / 4 : cap;
    if ((chunk < n ? chunk : n) <= 1024) {  // short lines: a wave each
      if (out) k_scan_row<T, false><<<(unsigned)g4, 256, 0, st>>>(a);
      else k_scan_row_totals<T, false><<<(unsigned)g4, 256, 0, st>>>(a);
    } else {
      if (out) k_scan_row<T, true><<<(unsigned)g1, 256, 0, st>>>(a);
      else k_scan_row_totals<T, true><<<(unsigned)g1, 256, 0, st>>>(a);
    }
  } else {
    const i64 items = outer * nc * ((inner + 63) / 64);
    const unsigned g = (unsigned)(items < cap ? items : cap);
    if (out) k_scan_col<T><<<g, 64 * SCAN_CW, 0, st>>>(a);
    else k_scan_col_totals<T><<<g, 64 * SCAN_CW, 0, st>>>(a);
  }
  LAUNCH_CHECK("spx_scan");
  return SPX_OK;
}

template <typename T>
static int scan_run(const void* in, void* out, i64 outer, i64 n, i64 inner, const void* carry, void* totals,
                    int exclusive, void* ws, hipStream_t st) {
  // the accumulator as an input type of its own: int64 -> int64, fp64 -> fp64
  typedef typename std::conditional<std::is_floating_point<T>::value, double, int64_t>::type AT;
  if (!scan_chunked(outer, n, inner))
    return scan_launch<T>(in, out, outer, n, inner, 1, n, carry, nullptr, totals, exclusive, st);
  const i64 nc = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
  // 1: chunk totals -> workspace
  int rc = scan_launch<T>(in, nullptr, outer, n, inner, nc, SCAN_CHUNK, nullptr, nullptr, ws, 0, st);
  if (rc != SPX_OK) return rc;
  // 2: exclusive scan of the chunk totals, in place (each segment is in
  // registers before it is stored); the line totals go to the caller
  rc = scan_launch<AT>(ws, out ? ws : nullptr, outer, nc, inner, 1, nc, nullptr, nullptr, totals, 1, st);
  if (rc != SPX_OK || !out) return rc;
  // 3: every chunk with its base
  return scan_launch<T>(in, out, outer, n, inner, nc, SCAN_CHUNK, carry, ws, nullptr, exclusive, st);
}

extern "C" int64_t spx_scan_workspace(int in_dtype, int64_t outer, int64_t n, int64_t inner) {
  if (!valid_dtype(in_dtype) || !scan_geom_ok(outer, n, inner)) return -1;
  if (!scan_chunked(outer, n, inner)) return 0;
  return outer * ((n + SCAN_CHUNK - 1) / SCAN_CHUNK) * inner * 8;
}

extern "C" int spx_scan(int in_dtype, const void* in, void* out, int64_t outer, int64_t n, int64_t inner,
                        const void* carry, void* totals, int exclusive, void* workspace,
                        size_t workspace_bytes, void* stream) {
  if (!valid_dtype(in_dtype)) return set_err(SPX_EINVAL, "spx_scan: bad dtype %d", in_dtype);
  if (!scan_geom_ok(outer, n, inner))
    return set_err(SPX_EINVAL, "spx_scan: bad geometry (outer %lld, n %lld, inner %lld)", (long long)outer,
                   (long long)n, (long long)inner);
  if (!in) return set_err(SPX_EINVAL, "spx_scan: null input");
  if (!out && !totals) return set_err(SPX_EINVAL, "spx_scan: out and totals are both null");
  const int64_t need = spx_scan_workspace(in_dtype, outer, n, inner);
  if (need > 0 && (!workspace || workspace_bytes < (size_t)need))
    return set_err(SPX_EINVAL, "spx_scan: workspace of %zu bytes, %lld needed", workspace_bytes, (long long)need);
  if (need > 0 && !scan_aligned(workspace, 8)) return set_err(SPX_EINVAL, "spx_scan: workspace not 8-byte aligned");
  hipStream_t st = S(stream);
  switch (in_dtype) {
    case SPX_BOOL: return scan_run<uint8_t>(in, out, outer, n, inner, carry, totals, exclusive, workspace, st);
    case SPX_I32: return scan_run<int32_t>(in, out, outer, n, inner, carry, totals, exclusive, workspace, st);
    case SPX_I64: return scan_run<int64_t>(in, out, outer, n, inner, carry, totals, exclusive, workspace, st);
    case SPX_F32: return scan_run<float>(in, out, outer, n, inner, carry, totals, exclusive, workspace, st);
    default: return scan_run<double>(in, out, outer, n, inner, carry, totals, exclusive, workspace, st);
  }
}

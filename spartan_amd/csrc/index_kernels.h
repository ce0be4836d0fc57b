// Index-array kernels behind spx_take / spx_compact_count / spx_compact
// (include/spx.h).  Included from spx.hip after scan_kernels.h (the tile
// table of a compaction is scanned by scan_run).
//
// Blocks are viewed as (outer, n, inner) as in spx_scan / spx_sort.  Values
// move as bit patterns of their element size (1 / 4 / 8 bytes), or as 16-byte
// vectors where the row bytes, the strides and the pointers allow it; a dtype
// only selects the size.  No atomics and no workgroup that waits for another:
// the same input gives the same bits.
//
// take: out[o, j, :] = src[o, idx[j] - lo, :] for the rows idx[j] (wrapped by
// n_total when negative) that fall into [lo, lo + n_local); the range test
// comes before any address is formed.
//   k_take_flat  rows shorter than 64 units (inner == 1 included): one lane
//     per output unit, index read and output write coalesced, the source
//     read random (L2 / Infinity Cache serve what locality the index has);
//   k_take_rows  longer rows: a wave (BLOCK: a workgroup, rows of 2048 units
//     and more) takes four rows at a time, lanes along the row, the four
//     loads issued before the four stores; row numbers are wave-uniform.
//
// compact: tiles of COMPACT_TILE mask bytes.  spx_compact_count counts every
// tile (k_compact_count: popcount of the nonzero-byte bits, the waves' sums
// met in LDS) into an int64 table, scans the table exclusively in place with
// scan_run and writes the total to a device word.  spx_compact reads the mask
// again: each wave takes a quarter of the tile in steps of 64 bytes, keeps
// the step's ballot in scalar registers, the four wave counts meet in LDS
// (plain stores, one barrier), and a selected lane's rank is the table's
// base + the lower waves' counts + the earlier steps' popcounts + the
// popcount of the ballot below the lane.
//   k_compact_elems (inner == 1): the selected lanes of a step store a
//     contiguous ascending run;
//   k_compact_rows  (inner > 1): the ranks index a list of the tile's
//     selected rows in LDS, and the workgroup copies those rows with lanes
//     along the row as k_take_rows does.

#ifndef COMPACT_TILE
#define COMPACT_TILE 4096                   // mask bytes per workgroup; a multiple of 256, at most 65536
#endif
#define COMPACT_STEPS (COMPACT_TILE / 256)  // 64-byte steps per wave
#define TAKE_WAVE_MIN 64                    // units per row from which a wave takes whole rows
#define TAKE_BLOCK_MIN 2048                 // ... and from which a workgroup splits a row

typedef uint32_t idx_v4 __attribute__((ext_vector_type(4)));  // the 16-byte unit

static int index_elem_size(int dtype) { return dtype == SPX_BOOL ? 1 : (dtype == SPX_I32 || dtype == SPX_F32) ? 4 : 8; }

// rows s[k] -> d[k] (k < 4; a null source skips the row), units [u0, u1),
// LANES lanes along the row: four loads in flight before the four stores
template <typename V, int LANES>
__device__ __forceinline__ void index_copy_rows4(const V* const (&s)[4], V* const (&d)[4], i64 u0, i64 u1, int tid) {
  for (i64 u = u0 + tid; u < u1; u += LANES) {
    V v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (s[k]) v[k] = s[k][u];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (s[k]) d[k][u] = v[k];
  }
}

// -------------------------------------------------------------------- take
struct TakeArgs {
  const void* src;
  const void* idx;
  void* out;
  int32_t* err;
  i64 outer, n_total, lo, n_local, m;
  i64 L;         // units per row
  i64 oos, ors;  // out strides in units
  int small;     // outer * m * L < 2^32: 32-bit index arithmetic
};

// the source row of output row j: -1 skip (another block's row), -2 out of range
template <typename I>
__device__ __forceinline__ i64 take_row(const TakeArgs& a, i64 j) {
  i64 r = (i64)((const I*)a.idx)[j];
  if (r < 0) r += a.n_total;
  if (r < 0 || r >= a.n_total) return -2;
  if (r < a.lo || r >= a.lo + a.n_local) return -1;
  return r - a.lo;
}

template <typename V, typename I, bool ELEM>
__global__ __launch_bounds__(256) void k_take_flat(TakeArgs a) {
  const V* src = (const V*)a.src;
  V* out = (V*)a.out;
  const i64 total = a.outer * a.m * a.L;
  for (i64 t = (i64)blockIdx.x * 256 + threadIdx.x; t < total; t += (i64)gridDim.x * 256) {
    i64 u = 0, q = t, j, o;
    if (a.small) {
      uint32_t q32 = (uint32_t)t;
      if (!ELEM) {
        u = q32 % (uint32_t)a.L;
        q32 /= (uint32_t)a.L;
      }
      j = q32 % (uint32_t)a.m;
      o = q32 / (uint32_t)a.m;
    } else {
      if (!ELEM) {
        u = t % a.L;
        q = t / a.L;
      }
      j = q % a.m;
      o = q / a.m;
    }
    const i64 r = take_row<I>(a, j);
    if (r == -2) {
      if (u == 0 && o == 0) *a.err = 1;
      continue;
    }
    if (r < 0) continue;
    out[o * a.oos + j * a.ors + u] = src[(o * a.n_local + r) * a.L + u];
  }
}

template <typename V, typename I, bool BLOCK>
__global__ __launch_bounds__(256) void k_take_rows(TakeArgs a) {
  constexpr int LANES = BLOCK ? 256 : 64;
  const int tid = BLOCK ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const i64 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 mg = (a.m + 3) / 4;  // groups of four rows
  const i64 items = a.outer * mg;
  const i64 first = BLOCK ? (i64)blockIdx.x : (i64)blockIdx.x * 4 + wave;
  const i64 step = BLOCK ? (i64)gridDim.x : (i64)gridDim.x * 4;
  for (i64 g = first; g < items; g += step) {
    const i64 o = g / mg, j0 = (g - o * mg) * 4;
    const V* s[4];
    V* d[4];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s[k] = nullptr;
      d[k] = nullptr;
      if (j0 + k < a.m) {
        const i64 r = take_row<I>(a, j0 + k);
        bad = bad || r == -2;
        if (r >= 0) {
          s[k] = (const V*)a.src + (o * a.n_local + r) * a.L;
          d[k] = (V*)a.out + o * a.oos + (j0 + k) * a.ors;
        }
      }
    }
    if (bad && tid == 0 && o == 0) *a.err = 1;
    index_copy_rows4<V, LANES>(s, d, 0, a.L, tid);
  }
}

template <typename V, typename I>
static int take_launch(const TakeArgs& a, hipStream_t st) {
  const i64 cap = (i64)1 << 20;
  if (a.L < TAKE_WAVE_MIN) {
    const i64 total = a.outer * a.m * a.L;
    const i64 b = (total + 255) / 256;
    const unsigned grid = (unsigned)(b < cap ? b : cap);
    if (a.L == 1) k_take_flat<V, I, true><<<grid, 256, 0, st>>>(a);
    else k_take_flat<V, I, false><<<grid, 256, 0, st>>>(a);
  } else {
    const i64 items = a.outer * ((a.m + 3) / 4);
    if (a.L < TAKE_BLOCK_MIN) {
      const i64 b = (items + 3) / 4;
      k_take_rows<V, I, false><<<(unsigned)(b < cap ? b : cap), 256, 0, st>>>(a);
    } else {
      k_take_rows<V, I, true><<<(unsigned)(items < cap ? items : cap), 256, 0, st>>>(a);
    }
  }
  LAUNCH_CHECK("spx_take");
  return SPX_OK;
}

template <typename V>
static int take_launch_idx(const TakeArgs& a, int idx_dtype, hipStream_t st) {
  return idx_dtype == SPX_I32 ? take_launch<V, int32_t>(a, st) : take_launch<V, int64_t>(a, st);
}

static bool index_mul_ok(i64 a, i64 b, i64 c) {
  const i64 lim = (i64)1 << 60;
  if (a < 0 || b < 0 || c < 0) return false;
  if (a == 0 || b == 0 || c == 0) return true;
  if (a > lim / b) return false;
  return a * b <= lim / c;
}

extern "C" int spx_take(int dtype, int idx_dtype, const void* src, const void* idx, void* out, int64_t outer,
                        int64_t n_total, int64_t lo, int64_t n_local, int64_t m, int64_t inner,
                        int64_t out_outer_stride, int64_t out_row_stride, int32_t* err, void* stream) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_take: bad dtype %d", dtype);
  if (idx_dtype != SPX_I32 && idx_dtype != SPX_I64)
    return set_err(SPX_EINVAL, "spx_take: bad index dtype %d (int32 / int64)", idx_dtype);
  if (n_total < 0 || lo < 0 || n_local < 0 || lo > n_total || n_local > n_total - lo || !index_mul_ok(outer, m, inner) ||
      !index_mul_ok(outer, n_local, inner))
    return set_err(SPX_EINVAL,
                   "spx_take: bad geometry (outer %lld, n_total %lld, lo %lld, n_local %lld, m %lld, inner %lld)",
                   (long long)outer, (long long)n_total, (long long)lo, (long long)n_local, (long long)m,
                   (long long)inner);
  if (out_row_stride < inner || out_outer_stride < 0 || (outer > 1 && m > 0 && out_outer_stride < inner))
    return set_err(SPX_EINVAL, "spx_take: bad out strides (%lld, %lld) for rows of %lld", (long long)out_outer_stride,
                   (long long)out_row_stride, (long long)inner);
  if (outer == 0 || m == 0 || inner == 0) return SPX_OK;
  if (!idx || !out || !err) return set_err(SPX_EINVAL, "spx_take: null idx, out or err");
  if (!src && n_local > 0) return set_err(SPX_EINVAL, "spx_take: null source");
  hipStream_t st = S(stream);
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), st));
  const i64 es = index_elem_size(dtype);
  TakeArgs a;
  a.src = src;
  a.idx = idx;
  a.out = out;
  a.err = err;
  a.outer = outer;
  a.n_total = n_total;
  a.lo = lo;
  a.n_local = n_local;
  a.m = m;
  const i64 per = 16 / es;  // elements per 16-byte vector
  const bool vec = inner % per == 0 && out_outer_stride % per == 0 && out_row_stride % per == 0 &&
                   scan_aligned(src, 16) && scan_aligned(out, 16);
  const i64 unit = vec ? per : 1;
  a.L = inner / unit;
  a.oos = out_outer_stride / unit;
  a.ors = out_row_stride / unit;
  a.small = outer * m * a.L < ((i64)1 << 32) ? 1 : 0;
  if (vec) return take_launch_idx<idx_v4>(a, idx_dtype, st);
  switch (es) {
    case 1: return take_launch_idx<uint8_t>(a, idx_dtype, st);
    case 4: return take_launch_idx<uint32_t>(a, idx_dtype, st);
    default: return take_launch_idx<u64>(a, idx_dtype, st);
  }
}

// ----------------------------------------------------------------- compact
struct CompactArgs {
  const void* in;
  const uint8_t* mask;
  void* out;
  const i64* base;  // exclusive scan of the tile counts
  i64* table;       // k_compact_count: the tile counts
  i64 outer, n, count;
  i64 L;            // units per row
  i64 S, Lc;        // k_compact_rows: column chunks per row and units per chunk
  int vec;          // k_compact_count: 16-byte mask loads are aligned
};

// number of nonzero bytes of a 32-bit word
__device__ __forceinline__ int compact_nz4(uint32_t w) {
  return __popc((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u);
}

__global__ __launch_bounds__(256) void k_compact_count(CompactArgs a) {
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i64 t0 = (i64)blockIdx.x * COMPACT_TILE;
  const i64 t1 = t0 + COMPACT_TILE < a.n ? t0 + COMPACT_TILE : a.n;
  int c = 0;
  for (i64 j = t0 + (i64)threadIdx.x * 16; j < t1; j += 256 * 16) {
    if (a.vec && j + 16 <= t1) {
      const idx_v4 v = *(const idx_v4*)(a.mask + j);
      c += (compact_nz4(v.x) + compact_nz4(v.y)) + (compact_nz4(v.z) + compact_nz4(v.w));
    } else {
      for (int k = 0; k < 16; ++k)
        if (j + k < t1) c += a.mask[j + k] != 0;
    }
  }
  // the wave's sum: popcounts of the ballots of the counter's bits (a lane counts at most COMPACT_TILE / 16)
  int w = 0;
#pragma unroll
  for (int b = 0; (1 << b) <= COMPACT_TILE / 16; ++b) w += __popcll(__ballot((c >> b) & 1)) << b;
  if (lane == 0) wcnt[wave] = w;
  __syncthreads();
  if (threadIdx.x == 0) a.table[blockIdx.x] = (i64)((wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]));
}

// the ballots of this wave's quarter of the tile and their count
__device__ __forceinline__ int compact_ballots(const CompactArgs& a, i64 w0, int lane, u64 (&b)[COMPACT_STEPS]) {
  int cnt = 0;
  uint8_t mb[COMPACT_STEPS];  // branch-free loads, all in flight together: past the end a lane reads byte 0
#pragma unroll
  for (int k = 0; k < COMPACT_STEPS; ++k) {
    const i64 j = w0 + k * 64 + lane;
    mb[k] = a.mask[j < a.n ? j : 0];
  }
#pragma unroll
  for (int k = 0; k < COMPACT_STEPS; ++k) {
    const i64 j = w0 + k * 64 + lane;
    b[k] = __ballot(j < a.n && mb[k] != 0);
    cnt += __popcll(b[k]);
  }
  return cnt;
}

__device__ __forceinline__ int compact_below(u64 m) {  // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

template <typename U>
__global__ __launch_bounds__(256) void k_compact_elems(CompactArgs a) {
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 tile = blockIdx.x;
  const i64 w0 = tile * COMPACT_TILE + (i64)wave * (COMPACT_TILE / 4);
  u64 b[COMPACT_STEPS];
  const int cnt = compact_ballots(a, w0, lane, b);
  if (lane == 0) wcnt[wave] = cnt;
  __syncthreads();
  i64 pos0 = a.base[tile];
  for (int w = 0; w < wave; ++w) pos0 += wcnt[w];
  for (i64 o = blockIdx.y; o < a.outer; o += gridDim.y) {
    const U* in = (const U*)a.in + o * a.n;
    U* out = (U*)a.out + o * a.count;
    // every step's load is issued before the first store: with a load and
    // its store per step inside the branch, a[mask] on 2^28 fp32 took 0.81 ms
    // at density 1/2 against 0.50 ms this way; a lane that
    // selects nothing reads element 0
    U v[COMPACT_STEPS];
#pragma unroll
    for (int k = 0; k < COMPACT_STEPS; ++k) v[k] = in[((b[k] >> lane) & 1) ? w0 + k * 64 + lane : 0];
    i64 pos = pos0;
#pragma unroll
    for (int k = 0; k < COMPACT_STEPS; ++k) {
      const u64 m = b[k];
      if ((m >> lane) & 1) {
        const i64 p = pos + compact_below(m);
        if (p < a.count) out[p] = v[k];
      }
      pos += __popcll(m);
    }
  }
}

template <typename V>
__global__ __launch_bounds__(256) void k_compact_rows(CompactArgs a) {
  __shared__ int wcnt[4];
  __shared__ uint16_t rows[COMPACT_TILE];  // the tile's selected rows, ascending
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 tile = blockIdx.x;
  const int wq = wave * (COMPACT_TILE / 4);
  const i64 t0 = tile * COMPACT_TILE;
  u64 b[COMPACT_STEPS];
  const int cnt = compact_ballots(a, t0 + wq, lane, b);
  if (lane == 0) wcnt[wave] = cnt;
  __syncthreads();
  int pos = 0;
  for (int w = 0; w < wave; ++w) pos += wcnt[w];
#pragma unroll
  for (int k = 0; k < COMPACT_STEPS; ++k) {
    const u64 m = b[k];
    if ((m >> lane) & 1) rows[pos + compact_below(m)] = (uint16_t)(wq + k * 64 + lane);
    pos += __popcll(m);
  }
  __syncthreads();
  const i64 base = a.base[tile];
  i64 total = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
  if (base + total > a.count) total = a.count > base ? a.count - base : 0;
  for (i64 y = blockIdx.y; y < a.outer * a.S; y += gridDim.y) {
    const i64 o = y / a.S, c = y - o * a.S;
    const i64 u0 = c * a.Lc, u1 = u0 + a.Lc < a.L ? u0 + a.Lc : a.L;
    const V* in = (const V*)a.in + (o * a.n + t0) * a.L;
    V* out = (V*)a.out + (o * a.count + base) * a.L;
    if (u1 - u0 >= 64) {  // a wave takes whole rows, four at a time
      for (i64 r0 = (i64)wave * 4; r0 < total; r0 += 16) {
        const V* s[4];
        V* d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool ok = r0 + k < total;
          s[k] = ok ? in + (i64)rows[ok ? r0 + k : 0] * a.L : nullptr;
          d[k] = ok ? out + (r0 + k) * a.L : nullptr;
        }
        index_copy_rows4<V, 64>(s, d, u0, u1, lane);
      }
    } else {  // short rows: one lane per unit
      const uint32_t W = (uint32_t)(u1 - u0), units = (uint32_t)total * W;
      for (uint32_t t = threadIdx.x; t < units; t += 256) {
        const uint32_t r = t / W, u = (uint32_t)u0 + (t - r * W);
        out[(i64)r * a.L + u] = in[(i64)rows[r] * a.L + u];
      }
    }
  }
}

static i64 compact_tiles(i64 n) { return (n + COMPACT_TILE - 1) / COMPACT_TILE; }

extern "C" int64_t spx_compact_workspace(int64_t n) {
  if (n < 0 || n > ((i64)1 << 60)) return -1;
  if (n == 0) return 0;
  const i64 nt = compact_tiles(n);
  const int64_t sw = spx_scan_workspace(SPX_I64, 1, nt, 1);
  return sw < 0 ? -1 : nt * 8 + sw;
}

extern "C" int spx_compact_count(const void* mask, int64_t n, int64_t* total, void* workspace, size_t bytes,
                                 void* stream) {
  const int64_t need = spx_compact_workspace(n);
  if (need < 0) return set_err(SPX_EINVAL, "spx_compact_count: bad length %lld", (long long)n);
  if (!total) return set_err(SPX_EINVAL, "spx_compact_count: null total");
  hipStream_t st = S(stream);
  if (n == 0) {  // nothing to count: the total is 0, no launch
    HIP_TRY(hipMemsetAsync(total, 0, sizeof(int64_t), st));
    return SPX_OK;
  }
  if (!mask) return set_err(SPX_EINVAL, "spx_compact_count: null mask");
  if (!workspace || bytes < (size_t)need)
    return set_err(SPX_EINVAL, "spx_compact_count: workspace of %zu bytes, %lld needed", bytes, (long long)need);
  if (!scan_aligned(workspace, 8) || !scan_aligned(total, 8))
    return set_err(SPX_EINVAL, "spx_compact_count: workspace or total not 8-byte aligned");
  const i64 nt = compact_tiles(n);
  if (nt > 0x7fffffff) return set_err(SPX_ENOTSUP, "spx_compact_count: %lld tiles", (long long)nt);
  CompactArgs a = {};
  a.mask = (const uint8_t*)mask;
  a.table = (i64*)workspace;
  a.n = n;
  a.vec = scan_aligned(mask, 16) ? 1 : 0;
  k_compact_count<<<(unsigned)nt, 256, 0, st>>>(a);
  LAUNCH_CHECK("spx_compact_count");
  return scan_run<int64_t>(workspace, workspace, 1, nt, 1, nullptr, total, 1, (char*)workspace + nt * 8, st);
}

template <typename V>
static int compact_launch(CompactArgs& a, bool rows, hipStream_t st) {
  const i64 nt = compact_tiles(a.n);
  if (!rows) {
    const unsigned gy = (unsigned)(a.outer < 1024 ? a.outer : 1024);
    k_compact_elems<V><<<dim3((unsigned)nt, gy), 256, 0, st>>>(a);
  } else {
    // column chunks: enough workgroups for two per CU when the tiles and outer blocks are few
    const i64 want = 2 * (i64)scan_num_cus();
    i64 S = 1;
    if (nt * a.outer < want) S = (want + nt * a.outer - 1) / (nt * a.outer);
    const i64 maxS = a.L / 64 > 0 ? a.L / 64 : 1;  // at least 64 units per chunk
    if (S > maxS) S = maxS;
    a.Lc = (a.L + S - 1) / S;
    a.S = (a.L + a.Lc - 1) / a.Lc;
    const i64 y = a.outer * a.S;
    k_compact_rows<V><<<dim3((unsigned)nt, (unsigned)(y < 1024 ? y : 1024)), 256, 0, st>>>(a);
  }
  LAUNCH_CHECK("spx_compact");
  return SPX_OK;
}

extern "C" int spx_compact(int dtype, const void* in, const void* mask, void* out, int64_t outer, int64_t n,
                           int64_t inner, int64_t count, const void* workspace, size_t bytes, void* stream) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_compact: bad dtype %d", dtype);
  if (!index_mul_ok(outer, n, inner) || count < 0 || count > n)
    return set_err(SPX_EINVAL, "spx_compact: bad geometry (outer %lld, n %lld, inner %lld, count %lld)",
                   (long long)outer, (long long)n, (long long)inner, (long long)count);
  const int64_t need = spx_compact_workspace(n);
  if (need < 0) return set_err(SPX_EINVAL, "spx_compact: bad length %lld", (long long)n);
  if (outer == 0 || n == 0 || inner == 0 || count == 0) return SPX_OK;
  if (!in || !mask || !out) return set_err(SPX_EINVAL, "spx_compact: null in, mask or out");
  if (!workspace || bytes < (size_t)need)
    return set_err(SPX_EINVAL, "spx_compact: workspace of %zu bytes, %lld needed", bytes, (long long)need);
  if (!scan_aligned(workspace, 8)) return set_err(SPX_EINVAL, "spx_compact: workspace not 8-byte aligned");
  if (compact_tiles(n) > 0x7fffffff) return set_err(SPX_ENOTSUP, "spx_compact: %lld tiles", (long long)compact_tiles(n));
  hipStream_t st = S(stream);
  const i64 es = index_elem_size(dtype);
  CompactArgs a = {};
  a.in = in;
  a.mask = (const uint8_t*)mask;
  a.out = out;
  a.base = (const i64*)workspace;
  a.outer = outer;
  a.n = n;
  a.count = count;
  a.L = inner;
  a.S = 1;
  a.Lc = inner;
  if (inner == 1) {
    switch (es) {
      case 1: return compact_launch<uint8_t>(a, false, st);
      case 4: return compact_launch<uint32_t>(a, false, st);
      default: return compact_launch<u64>(a, false, st);
    }
  }
  const i64 per = 16 / es;
  if (inner % per == 0 && scan_aligned(in, 16) && scan_aligned(out, 16)) {
    a.L = inner / per;
    return compact_launch<idx_v4>(a, true, st);
  }
  switch (es) {
    case 1: return compact_launch<uint8_t>(a, true, st);
    case 4: return compact_launch<uint32_t>(a, true, st);
    default: return compact_launch<u64>(a, true, st);
  }
}

// Sort / argsort kernels behind spx_sort / spx_sort_workspace / spx_sort_plan
// (include/spx.h).  Included from spx.hip after scan_kernels.h (the radix
// passes scan their digit counts with the scan kernels).
//
// The input is a dense row-major block viewed as (outer, n, inner); each of
// the outer * inner lines is sorted ascending along n, stably, in NumPy's
// order.  Every value is turned into an unsigned key whose integer order is
// the value order (SortT::key); the inverse (SortT::val) gives the bit
// pattern back, so the values written are a permutation of the input's bits.
// Two things are decided by the COMPARISON key (SortT::canon) and not by the
// stored key: -0.0 and +0.0 tie (the stored key keeps the sign, so the
// multiset of zero signs survives), and every NaN is stored as one key above
// +inf (its sign and payload are canonicalised).  Ties keep input order.
//
// Two paths:
//   k_sort_lds  (n <= SORT_LDS_MAX): a workgroup loads 2048 / P lines (P: n
//     rounded up to a power of two) into LDS, runs a bitonic network on the
//     composite (canonical key, position) -- distinct within a line, so the
//     network's result is the stable order -- and stores once.  No workspace.
//   radix (longer lines): least-significant-digit passes of SORT_BITS bits
//     over tiles of SORT_TILE keys, grid = (tiles of a line) x (lines).  A
//     pass is three launches: k_sort_hist (per-tile digit counts, LDS integer
//     atomics), the exclusive scan of the counts in (digit, tile) order per
//     line (scan_run, in place), and k_sort_scatter.  A key's rank among the
//     equal digits of its tile follows its fixed (sub-tile, wave, round, lane)
//     order, which is its order in the line: per-wave match masks from eight
//     ballots, the count of matching lanes below, per-wave digit counters in
//     LDS and one cross-wave exclusive scan per digit.  Passes ping-pong
//     between two key buffers (plus 32-bit positions when indices are wanted)
//     in the workspace; the first pass reads `in` and the last one writes the
//     outputs.  Strided lines (inner > 1) are transposed to line-major keys
//     before the passes and back into the outputs after them (two more passes
//     over the data, all accesses coalesced); the scatter stages each
//     sub-tile in LDS in its final order so that it stores runs, not keys.
// No workgroup waits for another inside a launch, there are no float atomics
// and the integer atomics only count: same input, same geometry, same bits.

#define SORT_LDS_MAX 2048  // longest line of the LDS path; LDS elements per workgroup
#define SORT_BITS 8
#define SORT_NDIG (1 << SORT_BITS)
#define SORT_ROUNDS 8                    // keys per lane and sub-tile
#define SORT_SUB (256 * SORT_ROUNDS)     // keys per sub-tile (4 waves x rounds x 64 lanes)
#define SORT_TILE (8 * SORT_SUB)         // keys per workgroup and pass: 16384

typedef uint32_t u32;

template <typename T> struct SortT;
template <> struct SortT<uint8_t> {
  typedef u32 K;
  static constexpr int PASSES = 1;
  static __device__ __forceinline__ K key(uint8_t v) { return v ? 1u : 0u; }
  static __device__ __forceinline__ uint8_t val(K k) { return (uint8_t)k; }
  static __device__ __forceinline__ K canon(K k) { return k; }
};
template <> struct SortT<int32_t> {
  typedef u32 K;
  static constexpr int PASSES = 4;
  static __device__ __forceinline__ K key(int32_t v) { return (u32)v ^ 0x80000000u; }
  static __device__ __forceinline__ int32_t val(K k) { return (int32_t)(k ^ 0x80000000u); }
  static __device__ __forceinline__ K canon(K k) { return k; }
};
template <> struct SortT<int64_t> {
  typedef u64 K;
  static constexpr int PASSES = 8;
  static __device__ __forceinline__ K key(int64_t v) { return (u64)v ^ 0x8000000000000000ull; }
  static __device__ __forceinline__ int64_t val(K k) { return (int64_t)(k ^ 0x8000000000000000ull); }
  static __device__ __forceinline__ K canon(K k) { return k; }
};
// floats: negative values flip every bit, the others the sign bit; -0.0 is
// stored as the key just below +0.0's and compares as +0.0's; NaNs are the
// largest key (its inverse, all ones below the sign, is a NaN)
template <> struct SortT<float> {
  typedef u32 K;
  static constexpr int PASSES = 4;
  static __device__ __forceinline__ K key(float v) {
    const u32 b = __float_as_uint(v);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    return (b >> 31) ? ~b : b ^ 0x80000000u;
  }
  static __device__ __forceinline__ float val(K k) {
    return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k);
  }
  static __device__ __forceinline__ K canon(K k) { return k == 0x7FFFFFFFu ? 0x80000000u : k; }
};
template <> struct SortT<double> {
  typedef u64 K;
  static constexpr int PASSES = 8;
  static __device__ __forceinline__ K key(double v) {
    const u64 b = (u64)__double_as_longlong(v);
    if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return ~0ull;
    return (b >> 63) ? ~b : b ^ 0x8000000000000000ull;
  }
  static __device__ __forceinline__ double val(K k) {
    return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k));
  }
  static __device__ __forceinline__ K canon(K k) {
    return k == 0x7FFFFFFFFFFFFFFFull ? 0x8000000000000000ull : k;
  }
};

struct SortArgs {
  const void* in;        // T, (outer, n, inner)
  void* out_vals;        // T or NULL
  i64* out_idx;          // or NULL
  const void* src_keys;  // K, (lines, n): a pass's input when it is not the first
  const u32* src_pos;
  void* dst_keys;        // a pass's output when it is not the last
  u32* dst_pos;
  i64* counts;           // (lines, SORT_NDIG, nt): digit counts, then their exclusive scan
  i64 outer, n, inner, nt;
  int shift, want_idx;
  int first;    // the pass's keys are in line order: a key's position is its row
  int from_in;  // the pass reads `in` (values) instead of src_keys
  int last;     // the pass writes out_vals / out_idx instead of dst_keys / dst_pos
};

// ------------------------------------------------------------ LDS path
// P: n rounded up to a power of two (>= 2); lpb = SORT_LDS_MAX / P lines per
// workgroup.  Slot l * P + r holds row r of the group's line l; rows >= n are
// padding that compares above every real element (largest key, position >= n).
template <typename T>
__global__ __launch_bounds__(256) void k_sort_lds(SortArgs a, int P, int lpb) {
  typedef typename SortT<T>::K K;
  __shared__ K keys[SORT_LDS_MAX];
  __shared__ u32 pos[SORT_LDS_MAX];
  const int tid = threadIdx.x;
  const int E = P * lpb;
  const i64 lines = a.outer * a.inner;
  const i64 groups = (lines + lpb - 1) / lpb;
  const T* in = (const T*)a.in;
  T* ov = (T*)a.out_vals;
  // inner > 1: consecutive lanes take consecutive lines (adjacent in memory)
  const bool by_line = a.inner > 1 && lpb > 1;
  for (i64 g = blockIdx.x; g < groups; g += gridDim.x) {
    const i64 line0 = g * lpb;
    for (int e = tid; e < E; e += 256) {
      const int l = by_line ? e % lpb : e / P;
      const int r = by_line ? e / lpb : e % P;
      const i64 line = line0 + l;
      K k = ~(K)0;
      if (line < lines && r < a.n) {
        const i64 o = line / a.inner, c = line - o * a.inner;
        k = SortT<T>::key(in[(o * a.n + r) * a.inner + c]);
      }
      keys[l * P + r] = k;
      pos[l * P + r] = (u32)r;
    }
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        __syncthreads();
        for (int x = tid; x < E / 2; x += 256) {
          const int i = 2 * x - (x & (j - 1)), p = i + j;
          const bool up = ((i & (P - 1)) & k) == 0;
          const K ki = keys[i], kp = keys[p];
          const u32 pi = pos[i], pp = pos[p];
          const K ci = SortT<T>::canon(ki), cp = SortT<T>::canon(kp);
          const bool p_lt_i = cp < ci || (cp == ci && pp < pi);
          if (p_lt_i == up) {
            keys[i] = kp;
            keys[p] = ki;
            pos[i] = pp;
            pos[p] = pi;
          }
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < E; e += 256) {
      const int l = by_line ? e % lpb : e / P;
      const int r = by_line ? e / lpb : e % P;
      const i64 line = line0 + l;
      if (line < lines && r < a.n) {
        const i64 o = line / a.inner, c = line - o * a.inner;
        const i64 at = (o * a.n + r) * a.inner + c;
        if (ov) ov[at] = SortT<T>::val(keys[l * P + r]);
        if (a.out_idx) a.out_idx[at] = (i64)pos[l * P + r];
      }
    }
    __syncthreads();  // the next group's loads overwrite the slots
  }
}

// ---------------------------------------------------------- radix path
// row r of line L (= o * inner + c) of a pass's input
template <typename T>
__device__ __forceinline__ typename SortT<T>::K sort_load(const SortArgs& a, i64 L, i64 o, i64 c, i64 r) {
  typedef typename SortT<T>::K K;
  if (a.from_in) return SortT<T>::key(((const T*)a.in)[(o * a.n + r) * a.inner + c]);
  return ((const K*)a.src_keys)[L * a.n + r];
}

// Strided lines (inner > 1) of the radix path: the values are turned into
// keys and transposed to line-major (outer * inner, n) before the passes
// (k_sort_keys_t: `in` -> dst_keys) and the last pass's keys and positions
// are transposed back into the outputs (k_sort_out_t: src_keys / src_pos ->
// out_vals / out_idx), 64 x 64 tiles through LDS, so that both sides of
// either copy are coalesced.
template <typename T>
__global__ __launch_bounds__(256) void k_sort_keys_t(SortArgs a) {
  typedef typename SortT<T>::K K;
  __shared__ K tk[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const i64 nr = (a.n + 63) / 64, nc = (a.inner + 63) / 64;
  const i64 items = a.outer * nr * nc;
  const T* in = (const T*)a.in;
  K* dst = (K*)a.dst_keys;
  for (i64 item = blockIdx.x; item < items; item += gridDim.x) {
    const i64 cb = item % nc, t = item / nc;
    const i64 rb = t % nr, o = t / nr;
    const i64 r0 = rb * 64, c0 = cb * 64;
    for (int y = ty; y < 64; y += 4) {
      const i64 r = r0 + y, c = c0 + tx;
      if (r < a.n && c < a.inner) tk[y][tx] = SortT<T>::key(in[(o * a.n + r) * a.inner + c]);
    }
    __syncthreads();
    for (int y = ty; y < 64; y += 4) {
      const i64 c = c0 + y, r = r0 + tx;
      if (r < a.n && c < a.inner) dst[(o * a.inner + c) * a.n + r] = tk[tx][y];
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_sort_out_t(SortArgs a) {
  typedef typename SortT<T>::K K;
  __shared__ K tk[64][65];
  __shared__ u32 tp[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const i64 nr = (a.n + 63) / 64, nc = (a.inner + 63) / 64;
  const i64 items = a.outer * nr * nc;
  const K* src = (const K*)a.src_keys;
  T* ov = (T*)a.out_vals;
  for (i64 item = blockIdx.x; item < items; item += gridDim.x) {
    const i64 cb = item % nc, t = item / nc;
    const i64 rb = t % nr, o = t / nr;
    const i64 r0 = rb * 64, c0 = cb * 64;
    for (int y = ty; y < 64; y += 4) {
      const i64 c = c0 + y, r = r0 + tx;
      if (r < a.n && c < a.inner) {
        const i64 at = (o * a.inner + c) * a.n + r;
        tk[y][tx] = src[at];
        if (a.want_idx) tp[y][tx] = a.src_pos[at];
      }
    }
    __syncthreads();
    for (int y = ty; y < 64; y += 4) {
      const i64 r = r0 + y, c = c0 + tx;
      if (r < a.n && c < a.inner) {
        const i64 at = (o * a.n + r) * a.inner + c;
        if (ov) ov[at] = SortT<T>::val(tk[tx][y]);
        if (a.out_idx) a.out_idx[at] = (i64)tp[tx][y];
      }
    }
    __syncthreads();
  }
}

template <typename T>
__device__ __forceinline__ int sort_digit(typename SortT<T>::K k, int shift) {
  return (int)((SortT<T>::canon(k) >> shift) & (SORT_NDIG - 1));
}

// counts[(L, digit, tile)] = keys of the tile with that digit
template <typename T>
__global__ __launch_bounds__(256) void k_sort_hist(SortArgs a) {
  typedef typename SortT<T>::K K;
  __shared__ unsigned h[SORT_NDIG];
  const int tid = threadIdx.x;
  const i64 items = a.outer * a.inner * a.nt;
  for (i64 item = blockIdx.x; item < items; item += gridDim.x) {
    const i64 L = item / a.nt, t = item - L * a.nt;
    const i64 o = L / a.inner, c = L - o * a.inner;
    const i64 r0 = t * SORT_TILE;
    const i64 r1 = r0 + SORT_TILE < a.n ? r0 + SORT_TILE : a.n;
    h[tid] = 0;
    __syncthreads();
    for (i64 r = r0 + tid; r < r1; r += 256) {
      const K k = sort_load<T>(a, L, o, c, r);
      atomicAdd(&h[sort_digit<T>(k, a.shift)], 1u);
    }
    __syncthreads();
    a.counts[(L * SORT_NDIG + tid) * a.nt + t] = (i64)h[tid];
  }
}

// counts now hold, per (line, digit, tile), the number of keys of the line
// that go before the tile's keys of that digit.  Thread d of the workgroup
// owns digit d: `run` is where the next sub-tile's first key of digit d goes.
// A sub-tile's keys are first put into LDS in their final order (by digit,
// then by their order in the line) and stored from there, so that
// consecutive lanes store consecutive keys of one digit's run.
template <typename T>
__global__ __launch_bounds__(256) void k_sort_scatter(SortArgs a) {
  typedef typename SortT<T>::K K;
  __shared__ unsigned wcnt[4][SORT_NDIG];  // keys per (wave, digit) of the sub-tile
  __shared__ u32 lbase[4][SORT_NDIG];      // slot of the first key of (wave, digit)
  __shared__ u32 gdelta[SORT_NDIG];        // slot + gdelta[digit] = position in the line
  __shared__ u32 wsum[4];
  __shared__ K skey[SORT_SUB];
  __shared__ u32 spos[SORT_SUB];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
  const i64 items = a.outer * a.inner * a.nt;
  for (i64 item = blockIdx.x; item < items; item += gridDim.x) {
    const i64 L = item / a.nt, t = item - L * a.nt;
    const i64 o = L / a.inner, c = L - o * a.inner;
    const i64 r0 = t * SORT_TILE;
    const i64 r1 = r0 + SORT_TILE < a.n ? r0 + SORT_TILE : a.n;
    u32 run = (u32)a.counts[(L * SORT_NDIG + tid) * a.nt + t];
    for (i64 s = r0; s < r1; s += SORT_SUB) {
      const int cnt = (int)(r1 - s < SORT_SUB ? r1 - s : SORT_SUB);  // keys of this sub-tile
#pragma unroll
      for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
      __syncthreads();
      const i64 w0 = s + (i64)wave * (64 * SORT_ROUNDS) + lane;
      K key[SORT_ROUNDS];
      u32 off[SORT_ROUNDS];
#pragma unroll
      for (int q = 0; q < SORT_ROUNDS; ++q) {
        const i64 r = w0 + q * 64;
        const bool valid = r < r1;
        key[q] = valid ? sort_load<T>(a, L, o, c, r) : (K)0;
        const int d = sort_digit<T>(key[q], a.shift);
        // lanes of this round whose digit equals mine
        u64 m = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
        for (int b = 0; b < SORT_BITS; ++b) {
          const bool bit = (d >> b) & 1;
          const u64 bal = __builtin_amdgcn_ballot_w64(bit);
          m &= bit ? bal : ~bal;
        }
        const int leader = m ? __builtin_ctzll(m) : 0;
        unsigned prev = 0;
        if (valid && lane == leader) prev = atomicAdd(&wcnt[wave][d], (unsigned)__builtin_popcountll(m));
        prev = __shfl(prev, leader, 64);
        off[q] = prev + (u32)__builtin_popcountll(m & below);
      }
      __syncthreads();
      // exclusive scan over the digits of the sub-tile's digit totals
      u32 c4[4];
      u32 tot = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        c4[w] = wcnt[w][tid];
        tot += c4[w];
      }
      const u32 inc = (u32)scan_wave_incl<u64>((u64)tot);
      if (lane == 63) wsum[wave] = inc;
      __syncthreads();
      {
        u32 lstart = inc - tot;
#pragma unroll
        for (int w = 0; w < 4; ++w)
          if (w < wave) lstart += wsum[w];
        gdelta[tid] = run - lstart;  // modulo 2^32; slot + gdelta is exact
        u32 b = lstart;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          lbase[w][tid] = b;
          b += c4[w];
        }
        run += tot;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < SORT_ROUNDS; ++q) {
        const i64 r = w0 + q * 64;
        if (r < r1) {
          const int d = sort_digit<T>(key[q], a.shift);
          const u32 slot = lbase[wave][d] + off[q];
          skey[slot] = key[q];
          if (a.want_idx) spos[slot] = a.first ? (u32)r : a.src_pos[L * a.n + r];
        }
      }
      __syncthreads();
      for (int j = tid; j < cnt; j += 256) {
        const K k = skey[j];
        const i64 dest = (i64)(u32)(gdelta[sort_digit<T>(k, a.shift)] + (u32)j);
        if (a.last) {
          const i64 at = (o * a.n + dest) * a.inner + c;
          if (a.out_vals) ((T*)a.out_vals)[at] = SortT<T>::val(k);
          if (a.out_idx) a.out_idx[at] = (i64)spos[j];
        } else {
          ((K*)a.dst_keys)[L * a.n + dest] = k;
          if (a.want_idx) a.dst_pos[L * a.n + dest] = spos[j];
        }
      }
      // the next sub-tile zeroes wcnt[.][tid], which only this thread read; two
      // barriers stand between these loads of skey / spos / gdelta and the
      // next stores to them
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ host
static int sort_passes(int dtype) {
  switch (dtype) {
    case SPX_BOOL: return SortT<uint8_t>::PASSES;
    case SPX_I32: return SortT<int32_t>::PASSES;
    case SPX_I64: return SortT<int64_t>::PASSES;
    case SPX_F32: return SortT<float>::PASSES;
    default: return SortT<double>::PASSES;
  }
}

static size_t sort_key_bytes(int dtype) { return dtype == SPX_I64 || dtype == SPX_F64 ? 8 : 4; }

// 0: fine; SPX_EINVAL / SPX_ENOTSUP otherwise
static int sort_geom_check(int dtype, i64 outer, i64 n, i64 inner) {
  if (!valid_dtype(dtype) || outer < 0 || n < 0 || inner < 0) return SPX_EINVAL;
  if (n >= ((i64)1 << 31)) return SPX_ENOTSUP;
  if (outer == 0 || n == 0 || inner == 0) return SPX_OK;
  const i64 lim = (i64)1 << 60;
  if (outer > lim / n || outer * n > lim / inner) return SPX_EINVAL;
  return SPX_OK;
}

static i64 sort_up256(i64 v) { return (v + 255) & ~(i64)255; }

// the radix path's workspace: counts | scan scratch | keys A | keys B | pos A | pos B
// (a single pass over contiguous lines goes from `in` to the outputs and needs
// no key buffer; strided lines always use both, for the two transposes)
struct SortWs {
  i64 counts, scan, keys[2], pos[2], total;
  i64 nt, scan_bytes;
};

static SortWs sort_layout(int dtype, i64 outer, i64 n, i64 inner, int want_idx) {
  SortWs w;
  const i64 lines = outer * inner, N = lines * n;
  const int passes = sort_passes(dtype);
  w.nt = (n + SORT_TILE - 1) / SORT_TILE;
  i64 at = 0;
  w.counts = at;
  at += sort_up256(lines * SORT_NDIG * w.nt * 8);
  w.scan_bytes = spx_scan_workspace(SPX_I64, lines, SORT_NDIG * w.nt, 1);
  if (w.scan_bytes < 0) w.scan_bytes = 0;
  w.scan = at;
  at += sort_up256(w.scan_bytes);
  for (int b = 0; b < 2; ++b) {
    w.keys[b] = at;
    if (passes > 1 + b || inner > 1) at += sort_up256(N * (i64)sort_key_bytes(dtype));
  }
  for (int b = 0; b < 2; ++b) {
    w.pos[b] = at;
    if (want_idx && (passes > 1 + b || inner > 1)) at += sort_up256(N * 4);
  }
  w.total = at;
  return w;
}

template <typename T>
static int sort_run(const void* in, void* out_vals, i64* out_idx, i64 outer, i64 n, i64 inner, int dtype,
                    void* ws, hipStream_t st) {
  const i64 lines = outer * inner;
  const i64 cap = (i64)1 << 20;
  SortArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in;
  a.out_vals = out_vals;
  a.out_idx = out_idx;
  a.outer = outer;
  a.n = n;
  a.inner = inner;
  a.want_idx = out_idx ? 1 : 0;
  if (n <= SORT_LDS_MAX) {
    int P = 2;
    while (P < n) P *= 2;
    const int lpb = SORT_LDS_MAX / P;
    const i64 groups = (lines + lpb - 1) / lpb;
    k_sort_lds<T><<<(unsigned)(groups < cap ? groups : cap), 256, 0, st>>>(a, P, lpb);
    LAUNCH_CHECK("spx_sort");
    return SPX_OK;
  }
  const SortWs w = sort_layout(dtype, outer, n, inner, a.want_idx);
  char* base = (char*)ws;
  a.nt = w.nt;
  a.counts = (i64*)(base + w.counts);
  const i64 items = lines * w.nt;
  const unsigned grid = (unsigned)(items < cap ? items : cap);
  const int passes = SortT<T>::PASSES;
  const bool tr = inner > 1;  // strided lines: transpose in, sort line-major, transpose out
  const i64 tiles64 = outer * ((n + 63) / 64) * ((inner + 63) / 64);
  const unsigned tgrid = (unsigned)(tiles64 < cap ? tiles64 : cap);
  if (tr) {
    a.dst_keys = base + w.keys[1];  // what pass 0 reads
    k_sort_keys_t<T><<<tgrid, 256, 0, st>>>(a);
    LAUNCH_CHECK("spx_sort");
    a.outer = lines;
    a.inner = 1;
  }
  for (int p = 0; p < passes; ++p) {
    a.shift = p * SORT_BITS;
    a.first = p == 0;
    a.from_in = !tr && p == 0;
    a.last = !tr && p == passes - 1;
    a.src_keys = base + w.keys[(p + 1) & 1];
    a.src_pos = (const u32*)(base + w.pos[(p + 1) & 1]);
    a.dst_keys = base + w.keys[p & 1];
    a.dst_pos = (u32*)(base + w.pos[p & 1]);
    k_sort_hist<T><<<grid, 256, 0, st>>>(a);
    LAUNCH_CHECK("spx_sort");
    const int rc = scan_run<int64_t>(a.counts, a.counts, lines, SORT_NDIG * w.nt, 1, nullptr, nullptr, 1,
                                     base + w.scan, st);
    if (rc != SPX_OK) return rc;
    k_sort_scatter<T><<<grid, 256, 0, st>>>(a);
    LAUNCH_CHECK("spx_sort");
  }
  if (tr) {
    a.outer = outer;
    a.inner = inner;
    a.src_keys = base + w.keys[(passes - 1) & 1];
    a.src_pos = (const u32*)(base + w.pos[(passes - 1) & 1]);
    k_sort_out_t<T><<<tgrid, 256, 0, st>>>(a);
    LAUNCH_CHECK("spx_sort");
  }
  return SPX_OK;
}

extern "C" int spx_sort_plan(int dtype, int64_t outer, int64_t n, int64_t inner, int64_t* lds_max,
                             int64_t* tile) {
  if (lds_max) *lds_max = SORT_LDS_MAX;
  if (tile) *tile = SORT_TILE;
  const int rc = sort_geom_check(dtype, outer, n, inner);
  if (rc != SPX_OK) return rc;
  return n <= SORT_LDS_MAX ? 0 : sort_passes(dtype);
}

extern "C" int64_t spx_sort_workspace(int dtype, int64_t outer, int64_t n, int64_t inner, int want_idx) {
  const int rc = sort_geom_check(dtype, outer, n, inner);
  if (rc != SPX_OK) return rc;
  if (n <= SORT_LDS_MAX || outer == 0 || inner == 0) return 0;
  return sort_layout(dtype, outer, n, inner, want_idx ? 1 : 0).total;
}

extern "C" int spx_sort(int dtype, const void* in, void* out_vals, int64_t* out_idx, int64_t outer, int64_t n,
                        int64_t inner, void* workspace, size_t workspace_bytes, void* stream) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_sort: bad dtype %d", dtype);
  const int rc = sort_geom_check(dtype, outer, n, inner);
  if (rc == SPX_ENOTSUP)
    return set_err(SPX_ENOTSUP, "spx_sort: lines of 2^31 or more elements are not supported (n %lld)",
                   (long long)n);
  if (rc != SPX_OK)
    return set_err(SPX_EINVAL, "spx_sort: bad geometry (outer %lld, n %lld, inner %lld)", (long long)outer,
                   (long long)n, (long long)inner);
  if (!in) return set_err(SPX_EINVAL, "spx_sort: null input");
  if (!out_vals && !out_idx) return set_err(SPX_EINVAL, "spx_sort: out_vals and out_idx are both null");
  if (in == out_vals || in == (const void*)out_idx)
    return set_err(SPX_EINVAL, "spx_sort: the input may not alias an output");
  const int64_t need = spx_sort_workspace(dtype, outer, n, inner, out_idx != nullptr);
  if (need > 0 && (!workspace || workspace_bytes < (size_t)need))
    return set_err(SPX_EINVAL, "spx_sort: workspace of %zu bytes, %lld needed", workspace_bytes, (long long)need);
  if (need > 0 && !scan_aligned(workspace, 8)) return set_err(SPX_EINVAL, "spx_sort: workspace not 8-byte aligned");
  if (outer == 0 || n == 0 || inner == 0) return SPX_OK;
  hipStream_t st = S(stream);
  switch (dtype) {
    case SPX_BOOL: return sort_run<uint8_t>(in, out_vals, out_idx, outer, n, inner, dtype, workspace, st);
    case SPX_I32: return sort_run<int32_t>(in, out_vals, out_idx, outer, n, inner, dtype, workspace, st);
    case SPX_I64: return sort_run<int64_t>(in, out_vals, out_idx, outer, n, inner, dtype, workspace, st);
    case SPX_F32: return sort_run<float>(in, out_vals, out_idx, outer, n, inner, dtype, workspace, st);
    default: return sort_run<double>(in, out_vals, out_idx, outer, n, inner, dtype, workspace, st);
  }
}

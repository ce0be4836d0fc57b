// Selection kernels behind spx_topk / spx_topk_workspace / spx_topk_plan and
// the fused nearest-neighbour search spx_knn / spx_knn_workspace /
// spx_knn_plan (include/spx.h).  Included from spx.hip after sort_kernels.h
// (SortT's order-preserving keys, SORT_LDS_MAX) and kmeans_kernels.h (k_cdist,
// whose tiling and addition order spx_knn repeats).
//
// topk.  The input is a dense row-major block viewed as (outer, n, inner);
// for each of the outer * inner lines the first k elements of the stable
// order are written to dense (outer, k, inner) outputs.  Every element gets
// an ORDER key (topk_ord): SortT's canonical key (-0.0 ties with +0.0, every
// NaN is one key above +inf) of the value for largest == 0; for largest != 0
// the key of the sign-flipped value for floats (NaNs stay last) and the
// inverted key for integers and bool (NumPy's ~x: no overflow at INT_MIN).
// The composite (order key, position) is distinct within a line, so "the first
// k" is well defined and every path below gives the same bits.  Values are
// read back from the input at the selected positions, so they carry the
// input's bit patterns (signs of zeros, NaN payloads).
//   lines of n <= SORT_LDS_MAX: k_topk_sort loads whole lines into LDS, runs
//     the bitonic network of k_sort_lds on (order key, position) and stores
//     only the first k.  No workspace.
//   longer lines: a most-significant-digit radix select, 8 bits a pass.  A
//     pass is three launches: k_topk_hist counts, per chunk of the line, the
//     digits of the keys that match the prefix found so far (LDS integer
//     atomics, one 256-bin table per chunk in the workspace), k_topk_pick
//     (one workgroup per line) adds the chunks' tables, finds the digit that
//     holds the k-th key and extends the prefix, and k_topk_fold (one wave per
//     chunk) adds to the chunk's counter the keys now known to be strictly
//     before the k-th key.  After the last
//     pass the prefix is the k-th key T; k_topk_compact reads the line once
//     more and writes, in position order (wave ballots, as k_compact), every
//     element before T and the first k - c elements equal to T (c: the keys
//     strictly before T) to a k-long candidate list; k_topk_sort orders the
//     candidates.  The line is read (key bytes + 1) times and never written;
//     strided lines (inner > 1) are indexed with their stride.
// No workgroup waits for another inside a launch; the integer atomics only
// count; there are no float atomics: same input, same geometry, same bits.

#define TOPK_K_MAX SORT_LDS_MAX   // the candidates of a line are ordered by one LDS sort
#define TOPK_CHUNK 16384          // elements of a line per workgroup of the select passes
#define TOPK_MAX_CHUNKS 1024      // longer lines get longer chunks (a multiple of 256)
template <typename T>
__device__ __forceinline__ typename SortT<T>::K topk_ord(T v, int largest) {
  typedef typename SortT<T>::K K;
  if constexpr (std::is_same<T, float>::value) {
    const u32 b = __float_as_uint(v) ^ (largest ? 0x80000000u : 0u);
    return SortT<T>::canon(SortT<T>::key(__uint_as_float(b)));
  } else if constexpr (std::is_same<T, double>::value) {
    const u64 b = (u64)__double_as_longlong(v) ^ (largest ? 0x8000000000000000ull : 0ull);
    return SortT<T>::canon(SortT<T>::key(__longlong_as_double((long long)b)));
  } else if constexpr (std::is_same<T, uint8_t>::value) {
    const K k = SortT<T>::key(v);
    return largest ? (k ^ (K)1) : k;
  } else {
    const K k = SortT<T>::key(v);
    return largest ? (K)~k : k;
  }
}

struct TopkState {  // per line, between the passes
  u64 prefix;       // the digits of the k-th key found so far (in place, low digits zero)
  u32 rank;         // 0-based rank of the k-th key among the keys that match the prefix
  u32 pad;
};

struct TopkArgs {
  const void* in;       // T, (outer, n, inner)
  const i64* in_idx;    // payload, in's shape, or NULL
  void* out_vals;       // T, (outer, k, inner), or NULL
  i64* out_idx;         // (outer, k, inner), or NULL
  TopkState* state;     // (lines)
  u32* hist;            // (lines, nch, 256)
  u32* less;            // (lines, nch): keys of the chunk strictly before the k-th key
  u32* eq;              // (lines, nch): keys of the chunk equal to the k-th key
  void* cand_key;       // K, (lines, k)
  u32* cand_pos;        // (lines, k)
  i64 outer, n, inner, k, chunk, nch;
  int shift, first, last, largest, from_cand;
};

// counts of digit (key >> shift) & 255 among the chunk's keys whose digits
// above it equal the prefix
template <typename T>
__global__ __launch_bounds__(256) void k_topk_hist(TopkArgs a) {
  typedef typename SortT<T>::K K;
  __shared__ unsigned h[256];
  const int tid = threadIdx.x;
  const i64 items = a.outer * a.inner * a.nch;
  const T* in = (const T*)a.in;
  for (i64 item = blockIdx.x; item < items; item += gridDim.x) {
    const i64 L = item / a.nch, ch = item - L * a.nch;
    const i64 o = L / a.inner, c = L - o * a.inner;
    const i64 r0 = ch * a.chunk;
    const i64 r1 = r0 + a.chunk < a.n ? r0 + a.chunk : a.n;
    const K pre = a.first ? (K)0 : (K)a.state[L].prefix;
    const int up = a.shift + 8;  // < the key's bits unless first
    h[tid] = 0;
    __syncthreads();
    for (i64 r = r0 + tid; r < r1; r += 256) {
      const K k = topk_ord<T>(in[(o * a.n + r) * a.inner + c], a.largest);
      if (a.first || (k >> up) == (pre >> up)) atomicAdd(&h[(unsigned)((k >> a.shift) & 255)], 1u);
    }
    __syncthreads();
    a.hist[(L * a.nch + ch) * 256 + tid] = h[tid];
    __syncthreads();
  }
}

// one workgroup per line; thread d owns digit d
__global__ __launch_bounds__(256) void k_topk_pick(TopkArgs a) {
  __shared__ u32 tot[256];
  __shared__ u32 sel[2];  // the digit, the rank within it
  const int tid = threadIdx.x;
  const i64 lines = a.outer * a.inner;
  for (i64 L = blockIdx.x; L < lines; L += gridDim.x) {
    const u32* hl = a.hist + L * a.nch * 256;
    u32 t = 0;
#pragma unroll 8
    for (i64 ch = 0; ch < a.nch; ++ch) t += hl[ch * 256 + tid];
    tot[tid] = t;
    __syncthreads();
    const u32 rank = a.first ? (u32)(a.k - 1) : a.state[L].rank;
    u32 cum = 0;
    for (int j = 0; j < tid; ++j) cum += tot[j];
    if (cum <= rank && rank - cum < t) {  // exactly one thread: the matching keys number more than rank
      sel[0] = (u32)tid;
      sel[1] = rank - cum;
    }
    __syncthreads();
    if (tid == 0) {
      TopkState st;
      st.prefix = (a.first ? 0ull : a.state[L].prefix) | ((u64)sel[0] << a.shift);
      st.rank = sel[1];
      st.pad = 0;
      a.state[L] = st;
    }
    __syncthreads();
  }
}

// one wave per (line, chunk), after the pick: the chunk's matching keys with a
// digit below the picked one are before the k-th key for good; the last pass
// also records the chunk's keys equal to it
__global__ __launch_bounds__(256) void k_topk_fold(TopkArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i64 items = a.outer * a.inner * a.nch;
  for (i64 item = (i64)blockIdx.x * 4 + wave; item < items; item += (i64)gridDim.x * 4) {  // wave-uniform
    const i64 L = item / a.nch;
    const u32 d = (u32)((a.state[L].prefix >> a.shift) & 255);
    const u32* hc = a.hist + item * 256;
    u32 s = 0;
    for (int j = lane; j < 256; j += 64)
      if ((u32)j < d) s += hc[j];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
      a.less[item] = a.first ? s : a.less[item] + s;
      if (a.last) a.eq[item] = hc[d];
    }
  }
}

// the k candidates of a line, in position order: every key before T and the
// first rank + 1 keys equal to T
template <typename T>
__global__ __launch_bounds__(256) void k_topk_compact(TopkArgs a) {
  typedef typename SortT<T>::K K;
  __shared__ u32 red[2][256];
  __shared__ u32 wl[4], we[4];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
  const i64 items = a.outer * a.inner * a.nch;
  const T* in = (const T*)a.in;
  K* ck = (K*)a.cand_key;
  for (i64 item = blockIdx.x; item < items; item += gridDim.x) {
    const i64 L = item / a.nch, ch = item - L * a.nch;
    const i64 o = L / a.inner, c = L - o * a.inner;
    const i64 r0 = ch * a.chunk;
    const i64 r1 = r0 + a.chunk < a.n ? r0 + a.chunk : a.n;
    const K Tk = (K)a.state[L].prefix;
    const u32 take = a.state[L].rank + 1;
    // keys before / equal to T in the chunks before this one
    u32 sl = 0, se = 0;
    for (i64 j = tid; j < ch; j += 256) {
      sl += a.less[L * a.nch + j];
      se += a.eq[L * a.nch + j];
    }
    red[0][tid] = sl;
    red[1][tid] = se;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        red[0][tid] += red[0][tid + s];
        red[1][tid] += red[1][tid + s];
      }
      __syncthreads();
    }
    u32 lrun = red[0][0], erun = red[1][0];
    const u32 mine_l = a.less[L * a.nch + ch], mine_e = a.eq[L * a.nch + ch];
    // nothing of this chunk is selected: no key before T, and the equal ones come too late
    const bool idle = mine_l == 0 && (mine_e == 0 || erun >= take);
    if (!idle) {
      for (i64 rb = r0; rb < r1; rb += 256) {  // block-uniform trip count
        const i64 r = rb + tid;
        const bool valid = r < r1;
        K k = 0;
        if (valid) k = topk_ord<T>(in[(o * a.n + r) * a.inner + c], a.largest);
        const bool isl = valid && k < Tk, ise = valid && k == Tk;
        const u64 ml = __builtin_amdgcn_ballot_w64(isl), me = __builtin_amdgcn_ballot_w64(ise);
        if (lane == 0) {
          wl[wave] = (u32)__builtin_popcountll(ml);
          we[wave] = (u32)__builtin_popcountll(me);
        }
        __syncthreads();
        u32 lb = lrun + (u32)__builtin_popcountll(ml & below);
        u32 eb = erun + (u32)__builtin_popcountll(me & below);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          if (w < wave) {
            lb += wl[w];
            eb += we[w];
          }
          lrun += wl[w];
          erun += we[w];
        }
        i64 slot = -1;
        if (isl) slot = (i64)lb + (eb < take ? eb : take);
        if (ise && eb < take) slot = (i64)lb + eb;
        if (slot >= 0 && slot < a.k) {
          ck[L * a.k + slot] = k;
          a.cand_pos[L * a.k + slot] = (u32)r;
        }
        __syncthreads();  // the next round overwrites wl / we
      }
    }
    __syncthreads();  // red is reused by the next item
  }
}

// Orders whole lines (from_cand == 0: m = n elements from `in`) or candidate
// lists (from_cand != 0: m = k (key, position) pairs) and writes the first k.
// P: m rounded up to a power of two (>= 2); lpb = SORT_LDS_MAX / P lines per
// workgroup; padding slots compare above every real element.
template <typename T>
__global__ __launch_bounds__(256) void k_topk_sort(TopkArgs a, int P, int lpb) {
  typedef typename SortT<T>::K K;
  __shared__ K keys[SORT_LDS_MAX];
  __shared__ u32 pos[SORT_LDS_MAX];
  const int tid = threadIdx.x;
  const int E = P * lpb;
  const i64 lines = a.outer * a.inner;
  const i64 groups = (lines + lpb - 1) / lpb;
  const i64 m = a.from_cand ? a.k : a.n;
  const T* in = (const T*)a.in;
  T* ov = (T*)a.out_vals;
  const K* ck = (const K*)a.cand_key;
  // inner > 1: consecutive lanes take consecutive lines (adjacent in memory)
  const bool by_line = a.inner > 1 && lpb > 1;
  for (i64 g = blockIdx.x; g < groups; g += gridDim.x) {
    const i64 line0 = g * lpb;
    for (int e = tid; e < E; e += 256) {
      const bool bl = by_line && !a.from_cand;
      const int l = bl ? e % lpb : e / P;
      const int r = bl ? e / lpb : e % P;
      const i64 line = line0 + l;
      K k = ~(K)0;
      u32 p = 0x80000000u | (u32)r;
      if (line < lines && r < m) {
        if (a.from_cand) {
          k = ck[line * a.k + r];
          p = a.cand_pos[line * a.k + r];
        } else {
          const i64 o = line / a.inner, c = line - o * a.inner;
          k = topk_ord<T>(in[(o * a.n + r) * a.inner + c], a.largest);
          p = (u32)r;
        }
      }
      keys[l * P + r] = k;
      pos[l * P + r] = p;
    }
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        __syncthreads();
        for (int x = tid; x < E / 2; x += 256) {
          const int i = 2 * x - (x & (j - 1)), p = i + j;
          const bool up = ((i & (P - 1)) & k) == 0;
          const K ki = keys[i], kp = keys[p];
          const u32 pi = pos[i], pp = pos[p];
          const bool p_lt_i = kp < ki || (kp == ki && pp < pi);
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
    const int kk = (int)a.k;
    for (int e = tid; e < kk * lpb; e += 256) {
      const int l = by_line ? e % lpb : e / kk;
      const int r = by_line ? e / lpb : e % kk;
      const i64 line = line0 + l;
      if (line < lines) {
        const i64 o = line / a.inner, c = line - o * a.inner;
        const u32 p = pos[l * P + r];  // r < k <= m: a real element
        const i64 src = (o * a.n + (i64)p) * a.inner + c;
        const i64 at = (o * a.k + r) * a.inner + c;
        if (p < (u32)a.n) {
          if (ov) ov[at] = in[src];
          if (a.out_idx) a.out_idx[at] = a.in_idx ? a.in_idx[src] : (i64)p;
        }
      }
    }
    __syncthreads();  // the next group's loads overwrite the slots
  }
}

// ------------------------------------------------------------------ host
static i64 topk_chunk(i64 n) {
  if (n <= (i64)TOPK_CHUNK * TOPK_MAX_CHUNKS) return TOPK_CHUNK;
  return ((n + TOPK_MAX_CHUNKS - 1) / TOPK_MAX_CHUNKS + 255) & ~(i64)255;
}

// 0: fine; SPX_EINVAL / SPX_ENOTSUP otherwise (k is checked by the callers)
static int topk_geom_check(int dtype, i64 outer, i64 n, i64 inner) { return sort_geom_check(dtype, outer, n, inner); }

// the select path's workspace: state | hist | less | eq | candidate keys | candidate positions
struct TopkWs {
  i64 state, hist, less, eq, ckey, cpos, total;
  i64 chunk, nch;
};

static TopkWs topk_layout(int dtype, i64 outer, i64 n, i64 inner, i64 k) {
  TopkWs w;
  const i64 lines = outer * inner;
  w.chunk = topk_chunk(n);
  w.nch = (n + w.chunk - 1) / w.chunk;
  i64 at = 0;
  w.state = at;
  at += sort_up256(lines * (i64)sizeof(TopkState));
  w.hist = at;
  at += sort_up256(lines * w.nch * 256 * 4);
  w.less = at;
  at += sort_up256(lines * w.nch * 4);
  w.eq = at;
  at += sort_up256(lines * w.nch * 4);
  w.ckey = at;
  at += sort_up256(lines * k * (i64)sort_key_bytes(dtype));
  w.cpos = at;
  at += sort_up256(lines * k * 4);
  w.total = at;
  return w;
}

template <typename T>
static int topk_run(const void* in, const i64* in_idx, void* out_vals, i64* out_idx, i64 outer, i64 n, i64 inner,
                    i64 k, int largest, int dtype, void* ws, hipStream_t st) {
  const i64 lines = outer * inner;
  const i64 cap = (i64)1 << 20;
  TopkArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in;
  a.in_idx = in_idx;
  a.out_vals = out_vals;
  a.out_idx = out_idx;
  a.outer = outer;
  a.n = n;
  a.inner = inner;
  a.k = k;
  a.largest = largest ? 1 : 0;
  if (n > SORT_LDS_MAX) {
    const TopkWs w = topk_layout(dtype, outer, n, inner, k);
    char* base = (char*)ws;
    a.state = (TopkState*)(base + w.state);
    a.hist = (u32*)(base + w.hist);
    a.less = (u32*)(base + w.less);
    a.eq = (u32*)(base + w.eq);
    a.cand_key = base + w.ckey;
    a.cand_pos = (u32*)(base + w.cpos);
    a.chunk = w.chunk;
    a.nch = w.nch;
    const i64 items = lines * w.nch;
    const unsigned grid = (unsigned)(items < cap ? items : cap);
    const unsigned lgrid = (unsigned)(lines < cap ? lines : cap);
    const unsigned fgrid = (unsigned)((items + 3) / 4 < cap ? (items + 3) / 4 : cap);
    const int passes = SortT<T>::PASSES;
    for (int p = 0; p < passes; ++p) {
      a.shift = (passes - 1 - p) * 8;
      a.first = p == 0;
      a.last = p == passes - 1;
      k_topk_hist<T><<<grid, 256, 0, st>>>(a);
      LAUNCH_CHECK("spx_topk");
      k_topk_pick<<<lgrid, 256, 0, st>>>(a);
      LAUNCH_CHECK("spx_topk");
      k_topk_fold<<<fgrid, 256, 0, st>>>(a);
      LAUNCH_CHECK("spx_topk");
    }
    k_topk_compact<T><<<grid, 256, 0, st>>>(a);
    LAUNCH_CHECK("spx_topk");
    a.from_cand = 1;
  }
  const i64 m = a.from_cand ? k : n;
  int P = 2;
  while (P < m) P *= 2;
  const int lpb = SORT_LDS_MAX / P;
  const i64 groups = (lines + lpb - 1) / lpb;
  k_topk_sort<T><<<(unsigned)(groups < cap ? groups : cap), 256, 0, st>>>(a, P, lpb);
  LAUNCH_CHECK("spx_topk");
  return SPX_OK;
}

static int topk_dispatch(int dtype, const void* in, const i64* in_idx, void* out_vals, i64* out_idx, i64 outer, i64 n,
                         i64 inner, i64 k, int largest, void* ws, hipStream_t st) {
  switch (dtype) {
    case SPX_BOOL: return topk_run<uint8_t>(in, in_idx, out_vals, out_idx, outer, n, inner, k, largest, dtype, ws, st);
    case SPX_I32: return topk_run<int32_t>(in, in_idx, out_vals, out_idx, outer, n, inner, k, largest, dtype, ws, st);
    case SPX_I64: return topk_run<int64_t>(in, in_idx, out_vals, out_idx, outer, n, inner, k, largest, dtype, ws, st);
    case SPX_F32: return topk_run<float>(in, in_idx, out_vals, out_idx, outer, n, inner, k, largest, dtype, ws, st);
    default: return topk_run<double>(in, in_idx, out_vals, out_idx, outer, n, inner, k, largest, dtype, ws, st);
  }
}

// 0: fine; also checks k.  Zero lines pass with any k >= 1 (nothing runs).
static int topk_check(int dtype, i64 outer, i64 n, i64 inner, i64 k) {
  const int rc = topk_geom_check(dtype, outer, n, inner);
  if (rc != SPX_OK) return rc;
  if (k < 1) return SPX_EINVAL;
  if (outer == 0 || inner == 0) return SPX_OK;
  if (k > n) return SPX_EINVAL;
  if (k > TOPK_K_MAX) return SPX_ENOTSUP;
  return SPX_OK;
}

extern "C" int spx_topk_plan(int dtype, int64_t outer, int64_t n, int64_t inner, int64_t k, int64_t* kmax,
                             int64_t* chunk) {
  if (kmax) *kmax = TOPK_K_MAX;
  if (chunk) *chunk = topk_chunk(n > 0 ? n : 1);
  const int rc = topk_check(dtype, outer, n, inner, k);
  if (rc != SPX_OK) return rc;
  return n <= SORT_LDS_MAX ? 0 : sort_passes(dtype);
}

extern "C" int64_t spx_topk_workspace(int dtype, int64_t outer, int64_t n, int64_t inner, int64_t k, int want_idx) {
  (void)want_idx;  // the candidates' positions are kept either way: the values are read through them
  const int rc = topk_check(dtype, outer, n, inner, k);
  if (rc != SPX_OK) return rc;
  if (n <= SORT_LDS_MAX || outer == 0 || inner == 0) return 0;
  return topk_layout(dtype, outer, n, inner, k).total;
}

extern "C" int spx_topk(int dtype, const void* in, const int64_t* in_idx, void* out_vals, int64_t* out_idx,
                        int64_t outer, int64_t n, int64_t inner, int64_t k, int largest, void* workspace,
                        size_t workspace_bytes, void* stream) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_topk: bad dtype %d", dtype);
  const int gc = topk_geom_check(dtype, outer, n, inner);
  if (gc == SPX_ENOTSUP)
    return set_err(SPX_ENOTSUP, "spx_topk: lines of 2^31 or more elements are not supported (n %lld)", (long long)n);
  if (gc != SPX_OK)
    return set_err(SPX_EINVAL, "spx_topk: bad geometry (outer %lld, n %lld, inner %lld)", (long long)outer,
                   (long long)n, (long long)inner);
  if (k < 1) return set_err(SPX_EINVAL, "spx_topk: k %lld is less than 1", (long long)k);
  if (!in) return set_err(SPX_EINVAL, "spx_topk: null input");
  if (!out_vals && !out_idx) return set_err(SPX_EINVAL, "spx_topk: out_vals and out_idx are both null");
  if (in == out_vals || in == (const void*)out_idx)
    return set_err(SPX_EINVAL, "spx_topk: the input may not alias an output");
  if (outer == 0 || inner == 0) return SPX_OK;
  if (k > n) return set_err(SPX_EINVAL, "spx_topk: k %lld exceeds the line length %lld", (long long)k, (long long)n);
  if (k > TOPK_K_MAX)
    return set_err(SPX_ENOTSUP, "spx_topk: k %lld exceeds the limit %d", (long long)k, (int)TOPK_K_MAX);
  const int64_t need = spx_topk_workspace(dtype, outer, n, inner, k, out_idx != nullptr);
  if (need > 0 && (!workspace || workspace_bytes < (size_t)need))
    return set_err(SPX_EINVAL, "spx_topk: workspace of %zu bytes, %lld needed", workspace_bytes, (long long)need);
  if (need > 0 && !scan_aligned(workspace, 8)) return set_err(SPX_EINVAL, "spx_topk: workspace not 8-byte aligned");
  return topk_dispatch(dtype, in, in_idx, out_vals, out_idx, outer, n, inner, k, largest, workspace, S(stream));
}

// ======================================================= nearest neighbours
// spx_knn: for each of Q fp64 queries the k points (of N, fp32 / fp64, row
// stride ldp) with the smallest (s, index), s the fp64 sum over d in order of
// (q[d] - x[d])^2 with every operation rounded separately -- k_cdist's value
// before its sqrt, the same tiling: a workgroup steps over 64-query x 64-point
// tiles, each lane 4 x 4 pairs, operands staged through LDS in 16-dim chunks
// (zero padding past D adds exact +0.0 terms).  The sums never leave the CU.
// Each query row of the workgroup keeps in LDS its best `kpad` entries (sorted,
// (orderable bits of s, point index)), the k-th of them as a threshold, and a
// buffer of `buf` entries.  A finished tile's sums are compared with the
// threshold; survivors are appended to the row's buffer (an LDS integer atomic
// hands out the slot: the order of arrival is arbitrary, the result is not,
// the composite key being a total order).  When a row's buffer is full the
// workgroup merges every row's buffer into its list with a bitonic network
// over kpad + buf entries (all comparators ascending, so a length that is not a
// power of two needs no padding), tightens the thresholds and the lanes retry
// what they could not append.  The points are cut into ranges of `chunk` over
// gridDim.y; each (query tile, range) writes its k entries to the workspace and
// a second step (the topk kernels above, on the int64 image of the keys with
// the indices as payload) selects per query among the ranges' lists: position
// order there is index order, so ties break by index.
#define KNN_K_MAX 128
#define KNN_T 64            // queries and points per tile
#define KNN_DC 16           // dims per staging step
#define KNN_CHUNK_MIN 2048  // points per (query tile, range) at least: a merge now and then, not per tile
#define KNN_BLOCKS 1024     // ranges are cut until about this many workgroups exist

// orderable bits of a sum: NaN -> one key above +inf's and below the empty slot's
__device__ __forceinline__ u64 knn_key(double s) {
  const u64 b = (u64)__double_as_longlong(s);
  if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return 0xFFF8000000000000ull;
  return (b >> 63) ? ~b : b ^ 0x8000000000000000ull;
}
// (ka, ia) before (kb, ib)
__device__ __forceinline__ bool knn_before(u64 ka, u32 ia, u64 kb, u32 ib) { return ka < kb || (ka == kb && ia < ib); }
#define KNN_EMPTY_KEY (~0ull)
#define KNN_EMPTY_IDX 0xFFFFFFFFu

struct KnnLds {  // byte offsets into the dynamic LDS block
  int qs, xs, ekey, eidx, tkey, tidx, cnt, total;
};
static __host__ __device__ inline KnnLds knn_lds(int M) {
  KnnLds l;
  int at = 0;
  l.qs = at;
  at += KNN_T * (KNN_DC + 1) * 8;
  l.xs = at;
  at += KNN_T * (KNN_DC + 1) * 8;
  l.ekey = at;
  at += KNN_T * M * 8;
  l.tkey = at;
  at += KNN_T * 8;
  l.eidx = at;
  at += KNN_T * M * 4;
  l.tidx = at;
  at += KNN_T * 4;
  l.cnt = at;
  at += KNN_T * 4;
  l.total = at;
  return l;
}

// every row's buffer merged into its list; thresholds and counts reset.  All
// 256 threads; the caller has a barrier between the last append and this.
__device__ __forceinline__ void knn_merge(u64* ekey, u32* eidx, u64* tkey, u32* tidx, u32* cnt, int M, int Mp,
                                          int kpad, int buf, int k) {
  const int tid = threadIdx.x;
  for (int e = tid; e < KNN_T * buf; e += 256) {
    const int row = e / buf, b = e - row * buf;
    if ((u32)b >= cnt[row]) {  // cnt may have run past buf: those lanes retry
      ekey[row * M + kpad + b] = KNN_EMPTY_KEY;
      eidx[row * M + kpad + b] = KNN_EMPTY_IDX;
    }
  }
  const int half = Mp >> 1;
  for (int kk = 2; kk <= Mp; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int e = tid; e < KNN_T * half; e += 256) {
        const int row = e / half, x = e - row * half;
        const int i = 2 * x - (x & (j - 1));
        // the first step of a merge mirrors within the block of kk, the others are half-cleaners
        const int p = (j == (kk >> 1)) ? (i ^ (kk - 1)) : (i + j);
        if (p < M) {
          u64* rk = ekey + row * M;
          u32* ri = eidx + row * M;
          const u64 ki = rk[i], kp = rk[p];
          const u32 ii = ri[i], ip = ri[p];
          if (knn_before(kp, ip, ki, ii)) {
            rk[i] = kp;
            rk[p] = ki;
            ri[i] = ip;
            ri[p] = ii;
          }
        }
      }
    }
  }
  __syncthreads();
  if (tid < KNN_T) {
    tkey[tid] = ekey[tid * M + k - 1];
    tidx[tid] = eidx[tid * M + k - 1];
    cnt[tid] = 0;
  }
  __syncthreads();
}

template <typename TP>
__global__ __launch_bounds__(256) void k_knn_tile(i64 Q, i64 N, i64 D, int k, const TP* __restrict__ X, i64 ldp,
                                                  const double* __restrict__ Qr, i64 index_base, i64 chunk,
                                                  i64 nch, int kpad, int buf, int Mp, i64* __restrict__ wkey,
                                                  i64* __restrict__ widx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_smem[];
  const int M = kpad + buf;
  const KnnLds lo = knn_lds(M);
  double(*Qs)[KNN_DC + 1] = (double(*)[KNN_DC + 1])(knn_smem + lo.qs);
  double(*Xs)[KNN_DC + 1] = (double(*)[KNN_DC + 1])(knn_smem + lo.xs);
  u64* ekey = (u64*)(knn_smem + lo.ekey);
  u32* eidx = (u32*)(knn_smem + lo.eidx);
  u64* tkey = (u64*)(knn_smem + lo.tkey);
  u32* tidx = (u32*)(knn_smem + lo.tidx);
  u32* cnt = (u32*)(knn_smem + lo.cnt);
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const i64 q0 = (i64)blockIdx.x * KNN_T;
  const i64 ch = blockIdx.y;
  const i64 j0 = ch * chunk;
  const i64 j1 = j0 + chunk < N ? j0 + chunk : N;
  for (int e = tid; e < KNN_T * M; e += 256) {
    ekey[e] = KNN_EMPTY_KEY;
    eidx[e] = KNN_EMPTY_IDX;
  }
  if (tid < KNN_T) {
    tkey[tid] = KNN_EMPTY_KEY;
    tidx[tid] = KNN_EMPTY_IDX;
    cnt[tid] = 0;
  }
  for (i64 p0 = j0; p0 < j1; p0 += KNN_T) {  // block-uniform
    double s[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[i][j] = 0.0;
    for (i64 d0 = 0; d0 < D; d0 += KNN_DC) {
      __syncthreads();
      for (int e = tid; e < KNN_T * KNN_DC; e += 256) {
        const int r = e / KNN_DC, dd = e % KNN_DC;
        Qs[r][dd] = (q0 + r < Q && d0 + dd < D) ? Qr[(q0 + r) * D + d0 + dd] : 0.0;
        Xs[r][dd] = (p0 + r < j1 && d0 + dd < D) ? (double)X[(p0 + r) * ldp + d0 + dd] : 0.0;
      }
      __syncthreads();
#pragma unroll 4
      for (int dd = 0; dd < KNN_DC; ++dd) {
        double q[4], x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          q[i] = Qs[ty + 16 * i][dd];
          x[i] = Xs[tx + 16 * i][dd];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double df = q[i] - x[j];
            const double sq = df * df;
            s[i][j] = s[i][j] + sq;
          }
      }
    }
    // survivors of the thresholds go to the rows' buffers; a full buffer: merge, retry
    u32 pend = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (q0 + ty + 16 * i < Q && p0 + tx + 16 * j < j1) pend |= 1u << (i * 4 + j);
    for (;;) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = ty + 16 * i;
        const u64 tk = tkey[row];
        const u32 ti = tidx[row];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const u32 bit = 1u << (i * 4 + j);
          if (pend & bit) {
            const u64 key = knn_key(s[i][j]);
            const u32 idx = (u32)(p0 + tx + 16 * j);
            if (!knn_before(key, idx, tk, ti)) {
              pend &= ~bit;
            } else {
              const u32 slot = atomicAdd(&cnt[row], 1u);
              if (slot < (u32)buf) {
                ekey[row * M + kpad + slot] = key;
                eidx[row * M + kpad + slot] = idx;
                pend &= ~bit;
              }
            }
          }
        }
      }
      if (!__syncthreads_or(pend != 0)) break;
      knn_merge(ekey, eidx, tkey, tidx, cnt, M, Mp, kpad, buf, k);
    }
  }
  __syncthreads();
  knn_merge(ekey, eidx, tkey, tidx, cnt, M, Mp, kpad, buf, k);
  for (int e = tid; e < KNN_T * k; e += 256) {
    const int row = e / k, r = e - row * k;
    const i64 q = q0 + row;
    if (q < Q) {
      const u64 key = ekey[row * M + r];
      const u32 idx = eidx[row * M + r];
      const i64 at = (q * nch + ch) * k + r;
      wkey[at] = (i64)(key ^ 0x8000000000000000ull);  // signed order = key order
      widx[at] = idx == KNN_EMPTY_IDX ? (i64)0x7FFFFFFFFFFFFFFFll : index_base + (i64)idx;
    }
  }
}

// out_s from the int64 image of the keys (and, with one range, the indices)
__global__ __launch_bounds__(256) void k_knn_finish(i64 n, const i64* __restrict__ keys, const i64* __restrict__ idx,
                                                    double* __restrict__ out_s, i64* __restrict__ out_idx) {
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
    const u64 key = (u64)keys[i] ^ 0x8000000000000000ull;
    const u64 b = (key >> 63) ? key ^ 0x8000000000000000ull : ~key;
    out_s[i] = __longlong_as_double((long long)b);
    if (idx) out_idx[i] = idx[i];
  }
}

struct KnnPlan {
  i64 chunk, nch;
  int kpad, buf, Mp;
  // workspace: range lists (keys, indices) | selected keys | the topk step's own
  i64 wkey, widx, skey, topk, total, topk_bytes;
};

static int knn_check(int dtype, i64 Q, i64 N, i64 D, i64 k) {
  if (dtype != SPX_F32 && dtype != SPX_F64) return SPX_ENOTSUP;
  if (Q < 0 || N < 0 || D < 1 || k < 1) return SPX_EINVAL;
  if (N >= ((i64)1 << 31)) return SPX_ENOTSUP;
  if (k > N) return SPX_EINVAL;
  if (k > KNN_K_MAX) return SPX_ENOTSUP;
  if (Q > ((i64)1 << 31) || D > ((i64)1 << 31)) return SPX_EINVAL;
  return SPX_OK;
}

static KnnPlan knn_plan(i64 Q, i64 N, i64 k) {
  KnnPlan p;
  const i64 qt = Q > 0 ? (Q + KNN_T - 1) / KNN_T : 1;
  const i64 want = qt >= KNN_BLOCKS ? 1 : KNN_BLOCKS / qt;
  i64 chunk = ((N + want - 1) / want + KNN_T - 1) / KNN_T * KNN_T;
  if (chunk < KNN_CHUNK_MIN) chunk = KNN_CHUNK_MIN;
  p.chunk = chunk;
  p.nch = N > 0 ? (N + chunk - 1) / chunk : 1;
  int kpad = 2;
  while (kpad < k) kpad *= 2;
  p.kpad = kpad;
  p.buf = kpad > 64 ? 32 : 64;  // 64 rows x (kpad + buf) entries of 12 bytes must fit the CU's LDS
  p.Mp = 2;
  while (p.Mp < kpad + p.buf) p.Mp *= 2;
  i64 at = 0;
  p.wkey = at;
  at += sort_up256(Q * p.nch * k * 8);
  p.widx = at;
  at += sort_up256(Q * p.nch * k * 8);
  p.skey = at;
  at += sort_up256(Q * k * 8);
  p.topk = at;
  p.topk_bytes = 0;
  if (p.nch > 1 && Q > 0) {
    const i64 t = spx_topk_workspace(SPX_I64, Q, p.nch * k, 1, k, 1);
    p.topk_bytes = t > 0 ? t : 0;
  }
  at += sort_up256(p.topk_bytes);
  p.total = at;
  return p;
}

extern "C" int spx_knn_plan(int dtype, int64_t Q, int64_t N, int64_t D, int64_t k, int64_t* kmax, int64_t* chunk) {
  if (kmax) *kmax = KNN_K_MAX;
  if (chunk) *chunk = knn_plan(Q > 0 ? Q : 1, N > 0 && N < ((i64)1 << 31) ? N : 1, 1).chunk;
  const int rc = knn_check(dtype, Q, N, D, k);
  if (rc != SPX_OK) return rc;
  return (int)knn_plan(Q, N, k).nch;
}

extern "C" int64_t spx_knn_workspace(int dtype, int64_t Q, int64_t N, int64_t D, int64_t k) {
  const int rc = knn_check(dtype, Q, N, D, k);
  if (rc != SPX_OK) return rc;
  if (Q == 0) return 0;
  return knn_plan(Q, N, k).total;
}

extern "C" int spx_knn(int dtype, int64_t Q, int64_t N, int64_t D, int64_t k, const void* points, int64_t ldp,
                       const double* queries, int64_t index_base, double* out_s, int64_t* out_idx, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (dtype != SPX_F32 && dtype != SPX_F64) return set_err(SPX_ENOTSUP, "spx_knn: points must be F32/F64");
  if (Q < 0 || N < 0 || D < 1 || ldp < D)
    return set_err(SPX_EINVAL, "spx_knn: bad sizes (Q %lld, N %lld, D %lld, ldp %lld)", (long long)Q, (long long)N,
                   (long long)D, (long long)ldp);
  if (N >= ((i64)1 << 31))
    return set_err(SPX_ENOTSUP, "spx_knn: 2^31 or more points are not supported (N %lld)", (long long)N);
  if (k < 1 || k > N) return set_err(SPX_EINVAL, "spx_knn: k %lld is outside [1, N = %lld]", (long long)k, (long long)N);
  if (k > KNN_K_MAX) return set_err(SPX_ENOTSUP, "spx_knn: k %lld exceeds the limit %d", (long long)k, KNN_K_MAX);
  if (knn_check(dtype, Q, N, D, k) != SPX_OK) return set_err(SPX_EINVAL, "spx_knn: bad sizes");
  if (!points || !queries || !out_s || !out_idx) return set_err(SPX_EINVAL, "spx_knn: null pointer");
  if (Q == 0) return SPX_OK;
  const KnnPlan p = knn_plan(Q, N, k);
  if (!workspace || workspace_bytes < (size_t)p.total)
    return set_err(SPX_EINVAL, "spx_knn: workspace of %zu bytes, %lld needed", workspace_bytes, (long long)p.total);
  if (!scan_aligned(workspace, 8)) return set_err(SPX_EINVAL, "spx_knn: workspace not 8-byte aligned");
  const i64 qt = (Q + KNN_T - 1) / KNN_T;
  if (p.nch > 65535) return set_err(SPX_ENOTSUP, "spx_knn: too many point ranges");
  hipStream_t st = S(stream);
  char* base = (char*)workspace;
  i64* wkey = (i64*)(base + p.wkey);
  i64* widx = (i64*)(base + p.widx);
  i64* skey = (i64*)(base + p.skey);
  const size_t lds = (size_t)knn_lds(p.kpad + p.buf).total;
  static bool attr = false;
  if (!attr) {
    const int most = knn_lds(KNN_K_MAX + 32).total > knn_lds(64 + 64).total ? knn_lds(KNN_K_MAX + 32).total
                                                                          : knn_lds(64 + 64).total;
    (void)hipFuncSetAttribute((const void*)k_knn_tile<float>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
    (void)hipFuncSetAttribute((const void*)k_knn_tile<double>, hipFuncAttributeMaxDynamicSharedMemorySize, most);
    attr = true;
  }
  dim3 grid((unsigned)qt, (unsigned)p.nch);
  if (dtype == SPX_F32)
    k_knn_tile<float><<<grid, 256, lds, st>>>(Q, N, D, (int)k, (const float*)points, ldp, queries, index_base, p.chunk,
                                              p.nch, p.kpad, p.buf, p.Mp, wkey, widx);
  else
    k_knn_tile<double><<<grid, 256, lds, st>>>(Q, N, D, (int)k, (const double*)points, ldp, queries, index_base,
                                               p.chunk, p.nch, p.kpad, p.buf, p.Mp, wkey, widx);
  LAUNCH_CHECK("spx_knn");
  const i64 n = Q * k;
  const i64 fb = (n + 255) / 256;
  const unsigned fgrid = (unsigned)(fb < 65536 ? fb : 65536);
  if (p.nch == 1) {
    k_knn_finish<<<fgrid, 256, 0, st>>>(n, wkey, widx, out_s, out_idx);
    LAUNCH_CHECK("spx_knn");
    return SPX_OK;
  }
  const int rc = topk_dispatch(SPX_I64, wkey, widx, skey, out_idx, Q, p.nch * k, 1, k, 0, base + p.topk, st);
  if (rc != SPX_OK) return rc;
  k_knn_finish<<<fgrid, 256, 0, st>>>(n, skey, nullptr, out_s, out_idx);
  LAUNCH_CHECK("spx_knn");
  return SPX_OK;
}

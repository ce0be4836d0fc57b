// Convolution and pooling kernels behind spx_stencil / spx_maxpool
// (include/spx.h).  Included from spx.hip after gemm_kernels.h (the MFMA
// fragment maps, spx_mfma::Mfma<T>).
//
// stencil: out[n, f, x, y] = sum over c, i, j with x + i < W and y + j < H of
// images[n, c, x + i, y + j] * filters[f, c, i, j] -- cross-correlation
// anchored at the top-left, taps past the bottom / right edge dropped.  Per
// image this is the product C = A B with M = F, N = W H, K = C fw fh:
//   A  the filter block as stored, (F, K) row-major;
//   B[k = (c, i, j)][col = x H + y] = images[n, c, x + i, y + j], or 0 where
//      the tap is clipped.  With col = x H + y the element sits at
//      c W H + col + i H + j of the image, so a row of B is a run of the
//      image shifted by i H + j, and the two clips are
//        x + i < W  <=>  col + i H < W H      (because y < H)
//        y + j < H                            (y = col mod H, once per thread)
//   C  the image's (F, W H) block of the output.
// B exists only in LDS.  k_stencil follows spx_mfma::gemm: block tile BM x BN,
// K-tiles of BK, WM x WN waves, A staged transposed (As[k][m]) and B row-major
// (Bs[k][n]) in two LDS buffers, the global loads of K-tile t + 1 issued
// before the MFMAs of tile t, one barrier per K-tile.  A thread stages ONE
// column of B (BN divides the block size; the threads of one column group
// share their rows), so its column, its y and its clips against the column
// are fixed for the whole K loop, and the row's (c, i, j) is block-uniform:
// it is stepped from row to row in scalar registers (no division in the
// loop).  Every predicate is decided before the address is formed: a load
// sits under its predicate and lands in a register that holds 0 (nothing is
// selected after the load, so no predicate stays live across the MFMAs and a
// K-tile's loads are all in flight together).  Rows past F, columns past
// W H and k past K stage 0 and are not stored.  One accumulation chain per
// element (K is a few thousand at most: gemm_kernels.h on chain lengths).
// No atomics, no workgroup that waits for another: the same input gives the
// same bits.
//
// maxpool: out[r, p, q] = max over i, j < pool with p s + i < W and q s + j <
// H of in[r, p s + i, q s + j], r over N C.  k_maxpool: one lane per output,
// lanes along H then W, reads clipped by predicate, no LDS.  The window's
// first element always exists, so there is no fill value; NaN propagates as
// in np.maximum (a NaN replaces the running maximum and is never replaced).

struct StencilArgs {
  const void* img;
  const void* flt;
  void* out;
  i64 N;
  uint32_t C, W, H, F, fw, fh;
  uint32_t K, WH;
  uint32_t tiles_n;
};

template <typename T, int BM, int BN, int BK, int WM, int WN>
__global__ __launch_bounds__(64 * WM* WN) void k_stencil(StencilArgs a) {
  typedef spx_mfma::Mfma<T> Fm;
  constexpr int NT = 64 * WM * WN;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / Fm::TILE, TN = WTN / Fm::TILE;
  constexpr int RG = NT / BN;         // thread groups that share a column of B
  constexpr int RB = BK / RG;         // rows of B per thread and K-tile
  constexpr int EA = BM * BK / NT;    // elements of A per thread and K-tile, consecutive in k
  constexpr int TPR = BK / EA;        // threads per row of A
  // fp64: B's rows padded to 32 dwords mod 64, so that the lane groups k and
  // k + 1 of a ds_read_b64 fall on different bank halves.  A's rows are NOT
  // padded (its transposing stores then meet 4-way on a bank, four stores per
  // thread and K-tile, and the fp64 A reads 2-way): without the pad the tiles
  // take 40960 / 53248 bytes, so that four (fp32) / three (fp64) workgroups
  // fit in a CU's 160 KiB instead of three / two
  constexpr int PADA = 0, PADB = sizeof(T) == 4 ? 0 : 16;
  static_assert(NT % BN == 0 && BN % 64 == 0 && BK % RG == 0, "a thread stages one column of B");
  static_assert((BM * BK) % NT == 0 && BK % EA == 0 && EA >= 1, "bad A staging");
  static_assert(TM >= 1 && TN >= 1 && BK % Fm::KS == 0, "bad wave tiling");
  __shared__ __attribute__((aligned(16))) T As[2][BK][BM + PADA];
  __shared__ __attribute__((aligned(16))) T Bs[2][BK][BN + PADB];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wm = w / WN, wn = w % WN;
  const uint32_t tm = blockIdx.x / a.tiles_n, tn = blockIdx.x - tm * a.tiles_n;
  const uint32_t row0 = tm * BM, col0 = tn * BN;
  const uint32_t K = a.K, WH = a.WH, H = a.H;
  // B staging: this thread's column and its row group (wave-uniform)
  const int cn = t % BN;
  const int rg = __builtin_amdgcn_readfirstlane(t / BN);
  const uint32_t col = col0 + cn;
  const bool colok = col < WH;
  const uint32_t y = col % H;
  // A staging: row ar, elements k0 + ak .. + EA
  const int ar = t / TPR, ak = (t % TPR) * EA;
  const bool arok = row0 + ar < a.F;
  const T* const arow = (const T*)a.flt + (i64)(arok ? row0 + ar : 0) * K;
  const int nk = (int)((K + BK - 1) / BK);
  for (i64 n = blockIdx.y; n < a.N; n += gridDim.y) {
    const T* const img = (const T*)a.img + n * a.C * (i64)WH;
    typename Fm::acc_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = Fm::zero();
    T ra[EA], rb[RB];
    // (c, i, j) of the next row of B to load, as cb = c W H and ih = i H: block-uniform
    uint32_t ki = 0, kj = 0, cb = 0, ih = 0;
    auto load = [&](uint32_t k0) {
#pragma unroll
      for (int e = 0; e < EA; ++e) {
        const uint32_t k = k0 + ak + e;
        T v = (T)0;
        if (arok && k < K) v = arow[k];
        ra[e] = v;
      }
#pragma unroll
      for (int r = 0; r < BK; ++r) {
        if (RG == 1 || r % RG == rg) {  // wave-uniform
          T v = (T)0;
          if (colok && k0 + r < K && col + ih < WH && y + kj < H) v = img[cb + ih + kj + col];
          rb[r / RG] = v;
        }
        if (++kj == a.fh) {
          kj = 0;
          ih += H;
          if (++ki == a.fw) {
            ki = 0;
            ih = 0;
            cb += WH;
          }
        }
      }
    };
    auto store = [&](int buf) {
#pragma unroll
      for (int e = 0; e < EA; ++e) As[buf][ak + e][ar] = ra[e];
#pragma unroll
      for (int q = 0; q < RB; ++q) Bs[buf][rg + RG * q][cn] = rb[q];
    };
    // opaque operands: the first tile's predicates and the epilogue's (both
    // invariant over the images) are not hoisted out of this loop, where they
    // would be held in scalar registers across the whole K loop
    uint32_t kz = 0;
    int fl = lane;
    asm volatile("" : "+s"(kz));
    load(kz);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) load((uint32_t)(kt + 1) * BK);
#pragma unroll
      for (int kk = 0; kk < BK / Fm::KS; ++kk) {
        const int k = kk * Fm::KS + Fm::opk(lane);
        T av[TM], bv[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) av[i] = As[cur][k][wm * WTM + i * Fm::TILE + Fm::opi(lane)];
#pragma unroll
        for (int j = 0; j < TN; ++j) bv[j] = Bs[cur][k][wn * WTN + j * Fm::TILE + Fm::opi(lane)];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = Fm::mma(av[i], bv[j], acc[i][j]);
      }
      if (kt + 1 < nk) store(cur ^ 1);
      __syncthreads();
    }
    T* const out = (T*)a.out + n * a.F * (i64)WH;
    asm volatile("" : "+v"(fl));
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < Fm::NREG; ++r) {
          const uint32_t gr = row0 + wm * WTM + i * Fm::TILE + Fm::crow(fl, r);
          const uint32_t gc = col0 + wn * WTN + j * Fm::TILE + Fm::ccol(fl);
          if (gr < a.F && gc < WH) out[(i64)gr * WH + gc] = acc[i][j][r];
        }
  }
}

// the block tiles: fp32 64 x 256 x 16 on 1 x 4 waves of 64 x 64 (2 x 2
// v_mfma_f32_32x32x2_f32 tiles); fp64 64 x 128 x 16 on 2 x 2 waves of 32 x 64
// (2 x 4 v_mfma_f64_16x16x4_f64 tiles)
template <typename T>
struct StencilTile;
template <>
struct StencilTile<float> {
  static constexpr int BM = 64, BN = 256, BK = 16, WM = 1, WN = 4;
};
template <>
struct StencilTile<double> {
  static constexpr int BM = 64, BN = 128, BK = 16, WM = 2, WN = 2;
};

template <typename T>
static int stencil_launch(StencilArgs& a, hipStream_t st) {
  typedef StencilTile<T> P;
  const i64 tiles_m = ((i64)a.F + P::BM - 1) / P::BM, tiles_n = ((i64)a.WH + P::BN - 1) / P::BN;
  if (tiles_m * tiles_n > 0x7fffffffLL)
    return set_err(SPX_ENOTSUP, "spx_stencil: %lld block tiles per image", (long long)(tiles_m * tiles_n));
  a.tiles_n = (uint32_t)tiles_n;
  const unsigned gy = (unsigned)(a.N < 65535 ? a.N : 65535);
  k_stencil<T, P::BM, P::BN, P::BK, P::WM, P::WN>
      <<<dim3((unsigned)(tiles_m * tiles_n), gy), 64 * P::WM * P::WN, 0, st>>>(a);
  LAUNCH_CHECK("spx_stencil");
  return SPX_OK;
}

extern "C" int spx_stencil_plan(int dtype, int64_t* bm, int64_t* bn, int64_t* bk) {
  if (dtype != SPX_F32 && dtype != SPX_F64)
    return set_err(SPX_EINVAL, "spx_stencil_plan: bad dtype %d (float32 / float64)", dtype);
  const bool f = dtype == SPX_F32;
  if (bm) *bm = f ? StencilTile<float>::BM : StencilTile<double>::BM;
  if (bn) *bn = f ? StencilTile<float>::BN : StencilTile<double>::BN;
  if (bk) *bk = f ? StencilTile<float>::BK : StencilTile<double>::BK;
  return SPX_OK;
}

extern "C" int spx_stencil(int dtype, const void* images, const void* filters, void* out, int64_t N, int64_t C,
                           int64_t W, int64_t H, int64_t F, int64_t fw, int64_t fh, void* stream) {
  if (dtype != SPX_F32 && dtype != SPX_F64)
    return set_err(SPX_EINVAL, "spx_stencil: bad dtype %d (float32 / float64)", dtype);
  if (N < 0 || C <= 0 || W <= 0 || H <= 0 || F <= 0 || fw <= 0 || fh <= 0)
    return set_err(SPX_EINVAL,
                   "spx_stencil: bad extent (N %lld, C %lld, W %lld, H %lld, F %lld, fw %lld, fh %lld)", (long long)N,
                   (long long)C, (long long)W, (long long)H, (long long)F, (long long)fw, (long long)fh);
  if (N == 0) return SPX_OK;
  if (!images || !filters || !out) return set_err(SPX_EINVAL, "spx_stencil: null images, filters or out");
  // the kernel's 32-bit indices: an image ((C + a K-tile's padding rows) W H),
  // an image's output block (F W H), the filter block (F K) and the largest
  // shift (fw H + fh) all stay below 2^31
  const i64 lim = (i64)1 << 31;
  const i64 pad = 16;
  if (W >= lim || H >= lim || C >= lim || F >= lim || fw >= lim || fh >= lim || W > lim / H ||
      C + pad > lim / (W * H) || F > lim / (W * H) || fw > lim / fh || C > lim / (fw * fh) ||
      F > lim / (C * fw * fh) || fw + 1 > lim / H || N > ((i64)1 << 60) / (W * H) / (C > F ? C : F))
    return set_err(SPX_ENOTSUP,
                   "spx_stencil: extents overflow 32-bit indices (N %lld, C %lld, W %lld, H %lld, F %lld, fw %lld, "
                   "fh %lld)", (long long)N, (long long)C, (long long)W, (long long)H, (long long)F, (long long)fw,
                   (long long)fh);
  StencilArgs a;
  a.img = images;
  a.flt = filters;
  a.out = out;
  a.N = N;
  a.C = (uint32_t)C;
  a.W = (uint32_t)W;
  a.H = (uint32_t)H;
  a.F = (uint32_t)F;
  a.fw = (uint32_t)fw;
  a.fh = (uint32_t)fh;
  a.K = (uint32_t)(C * fw * fh);
  a.WH = (uint32_t)(W * H);
  a.tiles_n = 0;
  return dtype == SPX_F32 ? stencil_launch<float>(a, S(stream)) : stencil_launch<double>(a, S(stream));
}

// ----------------------------------------------------------------- maxpool
struct PoolArgs {
  const void* in;
  void* out;
  i64 R, W, H, P, Q;  // R = N C planes of (W, H) -> (P, Q)
  i64 pool, stride;
  int small;          // R P Q < 2^32: 32-bit index arithmetic
};

template <typename T>
__global__ __launch_bounds__(256) void k_maxpool(PoolArgs a) {
  const T* in = (const T*)a.in;
  T* out = (T*)a.out;
  const i64 total = a.R * a.P * a.Q;
  for (i64 t = (i64)blockIdx.x * 256 + threadIdx.x; t < total; t += (i64)gridDim.x * 256) {
    i64 q, p, r;
    if (a.small) {
      uint32_t u = (uint32_t)t;
      const uint32_t row = u / (uint32_t)a.Q;
      q = u - row * (uint32_t)a.Q;
      const uint32_t rr = row / (uint32_t)a.P;
      p = row - rr * (uint32_t)a.P;
      r = rr;
    } else {
      const i64 row = t / a.Q;
      q = t - row * a.Q;
      r = row / a.P;
      p = row - r * a.P;
    }
    const i64 x0 = p * a.stride, y0 = q * a.stride;  // x0 < W and y0 < H: the window's first element exists
    const T* plane = in + r * a.W * a.H;
    T m = plane[x0 * a.H + y0];
    for (i64 i = 0; i < a.pool; ++i) {
      if (x0 + i >= a.W) break;
      for (i64 j = 0; j < a.pool; ++j) {
        if (y0 + j >= a.H) break;
        const T v = plane[(x0 + i) * a.H + y0 + j];
        m = (v > m || v != v) ? v : m;
      }
    }
    out[t] = m;
  }
}

template <typename T>
static int maxpool_launch(const PoolArgs& a, hipStream_t st) {
  const i64 total = a.R * a.P * a.Q, cap = (i64)1 << 20;
  const i64 b = (total + 255) / 256;
  k_maxpool<T><<<(unsigned)(b < cap ? b : cap), 256, 0, st>>>(a);
  LAUNCH_CHECK("spx_maxpool");
  return SPX_OK;
}

extern "C" int spx_maxpool(int dtype, const void* in, void* out, int64_t NC, int64_t W, int64_t H, int64_t pool,
                           int64_t stride, void* stream) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "spx_maxpool: bad dtype %d", dtype);
  if (NC < 0 || W <= 0 || H <= 0)
    return set_err(SPX_EINVAL, "spx_maxpool: bad extent (NC %lld, W %lld, H %lld)", (long long)NC, (long long)W,
                   (long long)H);
  if (pool < 1 || stride < 1)
    return set_err(SPX_EINVAL, "spx_maxpool: bad window (pool %lld, stride %lld)", (long long)pool, (long long)stride);
  if (NC == 0) return SPX_OK;
  if (!in || !out) return set_err(SPX_EINVAL, "spx_maxpool: null in or out");
  const i64 lim = (i64)1 << 60;
  if (W > lim / H || NC > lim / (W * H))
    return set_err(SPX_ENOTSUP, "spx_maxpool: extents overflow (NC %lld, W %lld, H %lld)", (long long)NC,
                   (long long)W, (long long)H);
  PoolArgs a;
  a.in = in;
  a.out = out;
  a.R = NC;
  a.W = W;
  a.H = H;
  a.P = (W - 1) / stride + 1;
  a.Q = (H - 1) / stride + 1;
  a.pool = pool < (W > H ? W : H) ? pool : (W > H ? W : H);  // a larger window is clipped to the plane anyway
  a.stride = stride;
  a.small = a.R * a.P * a.Q < ((i64)1 << 32) ? 1 : 0;
  hipStream_t st = S(stream);
  switch (dtype) {
    case SPX_BOOL: return maxpool_launch<uint8_t>(a, st);
    case SPX_I32: return maxpool_launch<int32_t>(a, st);
    case SPX_I64: return maxpool_launch<int64_t>(a, st);
    case SPX_F32: return maxpool_launch<float>(a, st);
    default: return maxpool_launch<double>(a, st);
  }
}

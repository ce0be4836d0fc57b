// sparse_kernels.h -- CSR x dense (spx_csrmm), CSR -> dense (spx_csr_todense) and
// the row number of every stored entry (spx_csr_rowids) for gfx950 (DESIGN.md
// 3.20, 3.22).  Included from spx.hip.
//
// C = alpha A B + beta C with A (m x n) in CSR (rowptr int64, col int32, val T)
// and B, C dense row-major.  The kernel is bound by the bytes of val / col and
// by the gather of B's rows, so its shape is chosen for the loads:
//
//   * a group of g lanes (a power of two up to 64, inside one wave) owns a row.
//     Of the g lanes, pl = min(g, pow2ceil(p)) lie along B's columns -- one
//     B row is read by pl adjacent lanes, coalesced -- and kl = g / pl along the
//     row's nonzeros (adjacent lanes read adjacent val / col).  p = 1 is the
//     "CSR-vector" SpMV.  Each lane sums its nonzeros k = kk, kk + kl, ... in
//     order; the kl sums are added by an xor butterfly (offsets pl, 2 pl, ...);
//   * a row of more than T nonzeros is cut into chunks of T.  A whole workgroup
//     sums one chunk (256 threads, the same pl / kl split with kl = 256 / pl, an
//     LDS tree in a fixed order) into a partial row in the workspace, and a
//     last kernel adds a row's partials in chunk order.  One very long row is
//     then spread over the chip instead of serialising on one CU.
//
// No float atomics: every element of C is written once by one lane, and its
// value is a fixed function of (the row's nonzeros, g, p).  The list of long
// rows and their chunks (the "analysis") is made by csr_find_long with an
// integer atomic cursor; the order of the list changes nothing that is summed.
// It depends on rowptr alone, lives at the head of the caller's workspace and
// is reused by every call with `prepared` set; the partial rows behind it are
// scratch of the call.
#pragma once

namespace spx_sp {

constexpr int BLOCK = 256;
constexpr i64 LONG_T = 2048;      // rows above this are cut into chunks of LONG_T
constexpr i64 HEADER = 64;        // bytes: [0] chunk cursor, [1] long-row cursor (u64)
constexpr int MAX_GRID = 1 << 20;

struct Item {  // one chunk of a long row
  i64 row, chunk;
};
struct LongRow {
  i64 row, first, count;  // its chunks are items first .. first + count - 1
};

struct Plan {
  int g, pl;
  i64 rows_cap, items_cap;
  i64 off_rows, off_items, off_part, total;  // bytes
};

static int pow2_floor(i64 v) {
  int r = 1;
  while (2 * (i64)r <= v && r < 64) r <<= 1;
  return r;
}

// pure host: the work shape of a problem.  g_hint (0: choose) lets the caller
// fix g, e.g. for all row slabs of one matrix.
static Plan make_plan(int es, i64 m, i64 nnz, i64 p, i64 g_hint) {
  Plan P;
  int pl = 1;
  while (pl < p && pl < 64) pl <<= 1;
  const i64 mean = m > 0 ? nnz / m : 0;
  i64 g = (i64)pow2_floor(mean < 1 ? 1 : mean) * pl;
  if (g > 64) g = 64;
  if (g_hint > 0) g = g_hint;
  if (pl > g) pl = (int)g;
  P.g = (int)g;
  P.pl = pl;
  P.rows_cap = std::min(m, nnz / (LONG_T + 1));
  P.items_cap = nnz / LONG_T + P.rows_cap;  // sum of ceil(len / T) over the long rows
  P.off_rows = HEADER;
  P.off_items = P.off_rows + P.rows_cap * (i64)sizeof(LongRow);
  P.off_part = P.off_items + P.items_cap * (i64)sizeof(Item);
  P.total = P.off_part + P.items_cap * (p < 1 ? 1 : p) * es;
  return P;
}

// ------------------------------------------------------------- analysis
__global__ __launch_bounds__(BLOCK) void csr_find_long(i64 m, const i64* __restrict__ rowptr,
                                                       unsigned long long* hdr, LongRow* rows, i64 rows_cap,
                                                       Item* items, i64 items_cap) {
  for (i64 r = (i64)blockIdx.x * BLOCK + threadIdx.x; r < m; r += (i64)gridDim.x * BLOCK) {
    const i64 len = rowptr[r + 1] - rowptr[r];
    if (len <= LONG_T) continue;
    const i64 nch = (len + LONG_T - 1) / LONG_T;
    const i64 first = (i64)atomicAdd(&hdr[0], (unsigned long long)nch);
    const i64 at = (i64)atomicAdd(&hdr[1], 1ull);
    if (at >= rows_cap || first + nch > items_cap) continue;  // a malformed rowptr: never past the lists
    rows[at].row = r;
    rows[at].first = first;
    rows[at].count = nch;
    for (i64 c = 0; c < nch; ++c) {
      items[first + c].row = r;
      items[first + c].chunk = c;
    }
  }
}

// ------------------------------------------------------------ short rows
template <typename T>
__global__ __launch_bounds__(BLOCK) void csrmm_rows(i64 m, i64 p, const i64* __restrict__ rowptr,
                                                    const int32_t* __restrict__ col, const T* __restrict__ val,
                                                    const T* __restrict__ B, i64 ldb, T* __restrict__ C, i64 ldc,
                                                    T alpha, T beta, int g, int pl, i64 nblocks) {
  const int tid = threadIdx.x;
  const int rpb = BLOCK / g;
  const int gl = tid & (g - 1);
  const int pj = gl & (pl - 1);
  const int kk = gl / pl;
  const int kl = g / pl;
  for (i64 rb = blockIdx.x; rb < nblocks; rb += gridDim.x) {  // uniform over the block
    const i64 r = rb * rpb + tid / g;
    i64 s = 0, e = 0;
    bool live = r < m;
    if (live) {
      s = rowptr[r];
      e = rowptr[r + 1];
      if (e - s > LONG_T) {  // the long-row kernels write this row
        live = false;
        e = s;
      }
    }
    for (i64 j0 = 0; j0 < p; j0 += pl) {
      const i64 j = j0 + pj;
      T acc = 0;
      if (j < p)
        for (i64 k = s + kk; k < e; k += kl) acc += val[k] * B[(i64)col[k] * ldb + j];
      for (int off = pl; off < g; off <<= 1) acc += __shfl_xor(acc, off);  // every lane of the wave
      if (live && kk == 0 && j < p) {
        T out = alpha * acc;
        if (beta != (T)0) out += beta * C[r * ldc + j];
        C[r * ldc + j] = out;
      }
    }
  }
}

// ------------------------------------------------------------- long rows
template <typename T>
__global__ __launch_bounds__(BLOCK) void csrmm_chunks(i64 p, const i64* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, const T* __restrict__ val,
                                                      const T* __restrict__ B, i64 ldb,
                                                      const unsigned long long* __restrict__ hdr,
                                                      const Item* __restrict__ items, i64 items_cap,
                                                      T* __restrict__ part, int pl) {
  __shared__ T red[BLOCK];
  const int tid = threadIdx.x;
  const int pj = tid & (pl - 1);
  const int kk = tid / pl;
  const int kl = BLOCK / pl;
  const i64 n_items = (i64)hdr[0];
  if (n_items > items_cap) return;  // a malformed rowptr overflowed the lists: nothing is trusted
  for (i64 it = blockIdx.x; it < n_items; it += gridDim.x) {
    const i64 r = items[it].row;
    const i64 s = rowptr[r] + items[it].chunk * LONG_T;
    const i64 e = rowptr[r + 1] < s + LONG_T ? rowptr[r + 1] : s + LONG_T;
    for (i64 j0 = 0; j0 < p; j0 += pl) {
      const i64 j = j0 + pj;
      T acc = 0;
      if (j < p)
        for (i64 k = s + kk; k < e; k += kl) acc += val[k] * B[(i64)col[k] * ldb + j];
      red[tid] = acc;
      __syncthreads();
      for (int st = BLOCK / 2; st >= pl; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
      }
      if (tid < pl && j < p) part[it * p + j] = red[tid];
      __syncthreads();
    }
  }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void csrmm_combine(i64 p, const unsigned long long* __restrict__ hdr,
                                                       const LongRow* __restrict__ rows, i64 rows_cap,
                                                       i64 items_cap, const T* __restrict__ part, T* __restrict__ C,
                                                       i64 ldc, T alpha, T beta) {
  const i64 n_rows = (i64)hdr[1];
  if (n_rows > rows_cap || (i64)hdr[0] > items_cap) return;
  for (i64 i = blockIdx.x; i < n_rows; i += gridDim.x) {
    const LongRow lr = rows[i];
    if (lr.first + lr.count > items_cap) continue;
    for (i64 j = threadIdx.x; j < p; j += BLOCK) {
      T acc = 0;
      for (i64 c = 0; c < lr.count; ++c) acc += part[(lr.first + c) * p + j];  // chunk order
      T out = alpha * acc;
      if (beta != (T)0) out += beta * C[lr.row * ldc + j];
      C[lr.row * ldc + j] = out;
    }
  }
}

template <typename T>
static hipError_t csrmm_run(const Plan& P, i64 m, i64 p, const i64* rowptr, const int32_t* col, const T* val,
                            const T* B, i64 ldb, T* C, i64 ldc, double alpha, double beta, char* ws, int prepared,
                            hipStream_t s) {
  unsigned long long* hdr = (unsigned long long*)ws;
  LongRow* rows = (LongRow*)(ws + P.off_rows);
  Item* items = (Item*)(ws + P.off_items);
  T* part = (T*)(ws + P.off_part);
  const bool longs = P.rows_cap > 0;
  if (longs && !prepared) {
    hipError_t e = hipMemsetAsync(hdr, 0, HEADER, s);
    if (e != hipSuccess) return e;
    const int grid = (int)std::min<i64>((m + BLOCK - 1) / BLOCK, MAX_GRID);
    hipLaunchKernelGGL(csr_find_long, dim3(grid), dim3(BLOCK), 0, s, m, rowptr, hdr, rows, P.rows_cap, items,
                       P.items_cap);
  }
  const int rpb = BLOCK / P.g;
  const i64 nblocks = (m + rpb - 1) / rpb;
  hipLaunchKernelGGL((csrmm_rows<T>), dim3((int)std::min<i64>(nblocks, MAX_GRID)), dim3(BLOCK), 0, s, m, p, rowptr,
                     col, val, B, ldb, C, ldc, (T)alpha, (T)beta, P.g, P.pl, nblocks);
  if (longs) {
    hipLaunchKernelGGL((csrmm_chunks<T>), dim3((int)std::min<i64>(P.items_cap, 1 << 16)), dim3(BLOCK), 0, s, p,
                       rowptr, col, val, B, ldb, hdr, items, P.items_cap, part, P.pl);
    hipLaunchKernelGGL((csrmm_combine<T>), dim3((int)std::min<i64>(P.rows_cap, 1 << 12)), dim3(BLOCK), 0, s, p, hdr,
                       rows, P.rows_cap, P.items_cap, part, C, ldc, (T)alpha, (T)beta);
  }
  return hipGetLastError();
}

// -------------------------------------------------------------- todense
template <typename T>
__global__ __launch_bounds__(BLOCK) void dense_zero(i64 m, i64 n, T* __restrict__ D, i64 ldd) {
  const i64 total = m * n;
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (i64)gridDim.x * BLOCK)
    D[(i / n) * ldd + i % n] = (T)0;
}

constexpr int DENSE_G = 16;  // lanes per row of the scatter

template <typename T>
__global__ __launch_bounds__(BLOCK) void csr_scatter(i64 m, i64 n, const i64* __restrict__ rowptr,
                                                     const int32_t* __restrict__ col, const T* __restrict__ val,
                                                     T* __restrict__ D, i64 ldd) {
  const i64 groups = (i64)gridDim.x * (BLOCK / DENSE_G);
  const int gl = threadIdx.x % DENSE_G;
  for (i64 r = (i64)blockIdx.x * (BLOCK / DENSE_G) + threadIdx.x / DENSE_G; r < m; r += groups) {
    const i64 e = rowptr[r + 1];
    for (i64 k = rowptr[r] + gl; k < e; k += DENSE_G) {
      const i64 c = col[k];
      if (c >= 0 && c < n) D[r * ldd + c] = val[k];  // a column outside the block is never written
    }
  }
}

template <typename T>
static hipError_t todense_run(i64 m, i64 n, const i64* rowptr, const int32_t* col, const T* val, T* D, i64 ldd,
                              hipStream_t s) {
  const i64 zb = (m * n + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL((dense_zero<T>), dim3((int)std::min<i64>(zb, MAX_GRID)), dim3(BLOCK), 0, s, m, n, D, ldd);
  const i64 sb = (m + BLOCK / DENSE_G - 1) / (BLOCK / DENSE_G);
  hipLaunchKernelGGL((csr_scatter<T>), dim3((int)std::min<i64>(sb, MAX_GRID)), dim3(BLOCK), 0, s, m, n, rowptr, col,
                     val, D, ldd);
  return hipGetLastError();
}

// -------------------------------------------------------------- row ids
// out[k] = r0 + i for every k in [rowptr[i], rowptr[i + 1]): the row number of
// every stored entry (the transpose's new column).  A wave per
// row, plain vector stores; an entry belongs to one row, so every word is
// written once.
__global__ __launch_bounds__(BLOCK) void csr_rowids(i64 m, i64 nnz, const i64* __restrict__ rowptr, i64 r0,
                                                    int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const i64 waves = (i64)gridDim.x * (BLOCK / 64);
  for (i64 r = (i64)blockIdx.x * (BLOCK / 64) + threadIdx.x / 64; r < m; r += waves) {
    i64 s = rowptr[r], e = rowptr[r + 1];
    if (s < 0) s = 0;  // a malformed rowptr: never outside out
    if (e > nnz) e = nnz;
    for (i64 k = s + lane; k < e; k += 64) out[k] = (int32_t)(r0 + r);
  }
}

}  // namespace spx_sp

// ------------------------------------------------------------------ C ABI
static const int64_t SP_MAX = (1LL << 40);

static int sp_check(const char* who, int dtype, int64_t m, int64_t nnz, int64_t p) {
  if (!valid_dtype(dtype)) return set_err(SPX_EINVAL, "%s: bad dtype %d", who, dtype);
  if (!linalg_dtype(dtype)) return set_err(SPX_ENOTSUP, "%s: dtype %d is not float32 / float64", who, dtype);
  if (m < 0 || nnz < 0 || p < 0)
    return set_err(SPX_EINVAL, "%s: negative size (m %lld, nnz %lld, p %lld)", who, (long long)m, (long long)nnz,
                   (long long)p);
  if (m > SP_MAX || nnz > SP_MAX || p > (1LL << 20))
    return set_err(SPX_ENOTSUP, "%s: size above the limit (m %lld, nnz %lld, p %lld)", who, (long long)m,
                   (long long)nnz, (long long)p);
  return SPX_OK;
}

extern "C" int spx_csrmm_plan(int dtype, int64_t m, int64_t nnz, int64_t p, int64_t* g, int64_t* long_row,
                              int64_t* rows_per_block) {
  int rc = sp_check("spx_csrmm_plan", dtype, m, nnz, p);
  if (rc != SPX_OK) return rc;
  const spx_sp::Plan P = spx_sp::make_plan(dtype == SPX_F32 ? 4 : 8, m, nnz, p, 0);
  if (g) *g = P.g;
  if (long_row) *long_row = spx_sp::LONG_T;
  if (rows_per_block) *rows_per_block = spx_sp::BLOCK / P.g;
  return SPX_OK;
}

extern "C" int64_t spx_csrmm_workspace(int dtype, int64_t m, int64_t nnz, int64_t p) {
  if (sp_check("spx_csrmm_workspace", dtype, m, nnz, p) != SPX_OK) return -1;
  return spx_sp::make_plan(dtype == SPX_F32 ? 4 : 8, m, nnz, p, 0).total;
}

extern "C" int spx_csrmm(int dtype, int64_t m, int64_t n, int64_t p, int64_t nnz, const int64_t* rowptr,
                         const int32_t* col, const void* val, const void* B, int64_t ldb, void* C, int64_t ldc,
                         double alpha, double beta, int64_t g, void* workspace, size_t workspace_bytes, int prepared,
                         void* stream) {
  int rc = sp_check("spx_csrmm", dtype, m, nnz, p);
  if (rc != SPX_OK) return rc;
  if (n < 0) return set_err(SPX_EINVAL, "spx_csrmm: negative size (n %lld)", (long long)n);
  if (n > 0x7fffffffLL) return set_err(SPX_ENOTSUP, "spx_csrmm: n = %lld is above the int32 column range", (long long)n);
  if (ldb < p || ldc < p)
    return set_err(SPX_EINVAL, "spx_csrmm: leading dimension (ldb %lld, ldc %lld) below p = %lld", (long long)ldb,
                   (long long)ldc, (long long)p);
  if (g != 0 && (g < 1 || g > 64 || (g & (g - 1))))
    return set_err(SPX_EINVAL, "spx_csrmm: g = %lld is not a power of two in 1 .. 64", (long long)g);
  if (m == 0 || p == 0) return SPX_OK;
  if (!rowptr || !C) return set_err(SPX_EINVAL, "spx_csrmm: null rowptr / C");
  if (nnz > 0 && (!col || !val || !B)) return set_err(SPX_EINVAL, "spx_csrmm: null col / val / B with nnz > 0");
  const spx_sp::Plan P = spx_sp::make_plan(dtype == SPX_F32 ? 4 : 8, m, nnz, p, g);
  if (P.rows_cap > 0 && (!workspace || (int64_t)workspace_bytes < P.total))
    return set_err(SPX_EINVAL, "spx_csrmm: workspace too small (%lld bytes needed)", (long long)P.total);
  hipError_t e = dtype == SPX_F32
                     ? spx_sp::csrmm_run<float>(P, m, p, rowptr, col, (const float*)val, (const float*)B, ldb,
                                                (float*)C, ldc, alpha, beta, (char*)workspace, prepared, S(stream))
                     : spx_sp::csrmm_run<double>(P, m, p, rowptr, col, (const double*)val, (const double*)B, ldb,
                                                 (double*)C, ldc, alpha, beta, (char*)workspace, prepared, S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_csrmm failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

extern "C" int spx_csr_todense(int dtype, int64_t m, int64_t n, int64_t nnz, const int64_t* rowptr,
                               const int32_t* col, const void* val, void* D, int64_t ldd, void* stream) {
  int rc = sp_check("spx_csr_todense", dtype, m, nnz, 1);
  if (rc != SPX_OK) return rc;
  if (n < 0) return set_err(SPX_EINVAL, "spx_csr_todense: negative size (n %lld)", (long long)n);
  if (n > 0x7fffffffLL)
    return set_err(SPX_ENOTSUP, "spx_csr_todense: n = %lld is above the int32 column range", (long long)n);
  if (ldd < n) return set_err(SPX_EINVAL, "spx_csr_todense: leading dimension %lld below n = %lld", (long long)ldd,
                              (long long)n);
  if (m == 0 || n == 0) return SPX_OK;
  if (!rowptr || !D) return set_err(SPX_EINVAL, "spx_csr_todense: null rowptr / D");
  if (nnz > 0 && (!col || !val)) return set_err(SPX_EINVAL, "spx_csr_todense: null col / val with nnz > 0");
  hipError_t e = dtype == SPX_F32 ? spx_sp::todense_run<float>(m, n, rowptr, col, (const float*)val, (float*)D, ldd,
                                                               S(stream))
                                  : spx_sp::todense_run<double>(m, n, rowptr, col, (const double*)val, (double*)D,
                                                                ldd, S(stream));
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_csr_todense failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

extern "C" int spx_csr_rowids(int64_t m, int64_t nnz, const int64_t* rowptr, int64_t r0, int32_t* out, void* stream) {
  if (m < 0 || nnz < 0 || r0 < 0)
    return set_err(SPX_EINVAL, "spx_csr_rowids: negative size (m %lld, nnz %lld, r0 %lld)", (long long)m,
                   (long long)nnz, (long long)r0);
  if (m > SP_MAX || nnz > SP_MAX || r0 > SP_MAX || r0 + m > 0x7fffffffLL)
    return set_err(SPX_ENOTSUP, "spx_csr_rowids: rows %lld .. %lld are above the int32 range", (long long)r0,
                   (long long)(r0 + m));
  if (m == 0 || nnz == 0) return SPX_OK;
  if (!rowptr || !out) return set_err(SPX_EINVAL, "spx_csr_rowids: null rowptr / out");
  const i64 blocks = (m + spx_sp::BLOCK / 64 - 1) / (spx_sp::BLOCK / 64);
  hipLaunchKernelGGL(spx_sp::csr_rowids, dim3((int)std::min<i64>(blocks, spx_sp::MAX_GRID)), dim3(spx_sp::BLOCK), 0,
                     S(stream), m, nnz, rowptr, r0, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_err(SPX_EHIP, "spx_csr_rowids failed: %s", hipGetErrorString(e));
  return SPX_OK;
}

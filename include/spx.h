/*
 * spx.h -- C ABI of libspx.so, the MI355X (gfx950) tile-execution backend
 * underneath spartan_amd.expr.
 *
 * The reference (sdutheone/spartan) has no native boundary on its hot path:
 * every tile operation is a NumPy/BLAS call made from a Python worker
 * (spartan/expr/local.py:110-122, spartan/expr/dot.py:195-212) and tiles move
 * over pickled ZeroMQ RPC.  Each entry point below replaces one of those
 * per-tile call sites; the reference interface it replaces is cited on it.
 *
 * Conventions
 *   - Every function returns 0 on success and a negative SPX_E* code on error;
 *     spx_last_error() returns the message of the calling thread's last error.
 *   - All device memory is owned by the caller (allocated through PyTorch-ROCm
 *     on the GPU of this rank).  The library never frees caller buffers.
 *   - Every compute call is asynchronous on the given hipStream_t (passed as
 *     void*; NULL = the null stream).  Nothing here synchronises the host.
 *   - Shapes, offsets and strides are in ELEMENTS, int64, row-major.
 *   - No torch types cross this boundary: plain pointers and sizes only.
 */
#ifndef SPX_H
#define SPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPX_ABI_VERSION 3  /* 2: spx_kmeans_assign dist_dtype; collectives; 3: spx_kmeans_step */
/* additive since 3 (no existing signature changed): spx_scan_workspace, spx_scan,
 * spx_sort_workspace, spx_sort, spx_sort_plan, spx_take, spx_compact_workspace,
 * spx_compact_count, spx_compact, spx_stencil_plan, spx_stencil, spx_maxpool,
 * spx_topk_workspace, spx_topk, spx_topk_plan, spx_knn_workspace, spx_knn, spx_knn_plan,
 * spx_potrf_plan, spx_potrf_workspace, spx_potrf, spx_trsm_workspace, spx_trsm, spx_syrk,
 * spx_geqr_plan, spx_geqr_workspace, spx_geqr, spx_orgqr, spx_csrmm_plan, spx_csrmm_workspace,
 * spx_csrmm, spx_csr_todense, spx_syevj_plan, spx_syevj, spx_gemm_plan, spx_csr_rowids,
 * spx_als_plan, spx_als_solve, spx_apsp_plan, spx_apsp, spx_fuzzy_plan, spx_fuzzy_step,
 * spx_gesvj_plan, spx_gesvj, spx_nbody_plan, spx_nbody_accel, spx_pairwise_plan,
 * spx_pairwise */

/* error codes */
#define SPX_OK 0
#define SPX_EINVAL -1   /* bad argument (shape / dtype / null pointer)      */
#define SPX_EHIP -2     /* HIP runtime error (message has hipGetErrorString) */
#define SPX_ENOTSUP -3  /* combination not supported by this build           */

/* element types (NumPy dtype on the Python side) */
#define SPX_BOOL 0 /* numpy.bool_  stored as uint8 0/1 */
#define SPX_I32 1  /* numpy.int32  */
#define SPX_I64 2  /* numpy.int64  */
#define SPX_F32 3  /* numpy.float32 */
#define SPX_F64 4  /* numpy.float64 */

/* reduction / merge operators (reference accumulate_fn / reducer) */
#define SPX_OP_SUM 0     /* np.add     */
#define SPX_OP_MIN 1     /* np.minimum */
#define SPX_OP_MAX 2     /* np.maximum */
#define SPX_OP_ARGMIN 3  /* (value, first index) min */
#define SPX_OP_ARGMAX 4  /* (value, first index) max */
#define SPX_OP_REPLACE 5 /* reducer None: last write wins */

/* fill kinds */
#define SPX_FILL_CONST 0   /* value a                                   */
#define SPX_FILL_ARANGE 1  /* a + b * global_flat_index                 */
#define SPX_FILL_UNIFORM 2 /* a + (b-a) * U[0,1) from splitmix64(seed,i) */
#define SPX_FILL_NORMAL 3  /* a + b * N(0,1), Box-Muller of streams 2i, 2i+1 */

/* ---------------------------------------------------------------- basics */
int spx_abi_version(void);
const char* spx_last_error(void);

/* ------------------------------------------------------------------- JIT
 * Fused map / map+reduce kernels are generated from the LocalExpr tree by
 * spartan_amd/codegen.py, compiled to a gfx950 code object, and launched
 * through these three calls.  Replaces FnCallExpr.evaluate
 * (spartan/expr/local.py:110-122) driven by tile_mapper (spartan/expr/map.py:48-88)
 * and _reduce_mapper (spartan/expr/reduce.py:19-68); the reference's own
 * codegen hook is ParakeetExpr (spartan/expr/local.py:154-200).
 */
int spx_module_load(const void* image, size_t nbytes, void** module_out);
int spx_module_unload(void* module);
int spx_module_function(void* module, const char* name, void** fn_out);
/* args points to the packed kernel-argument struct (copied by the runtime). */
int spx_launch(void* fn, uint32_t grid_x, uint32_t grid_y, uint32_t grid_z,
               uint32_t block_x, uint32_t shared_bytes, const void* args,
               size_t args_bytes, void* stream);

/* ------------------------------------------------------------------ fills
 * Replaces builtins._make_ones/_make_zeros (spartan/expr/builtins.py:370-375),
 * _arange_mapper (:404-411) and np.random.rand per tile (:29-31; the
 * reference RNG is not reproducible, ours is counter-based on the GLOBAL flat
 * index, so values do not depend on the tiling).
 * The tile is dense row-major with tile_shape; it sits at ul inside an array
 * of array_shape (ndim <= 8).
 */
int spx_fill(int dtype, int kind, void* out, int ndim, const int64_t* tile_shape,
             const int64_t* ul, const int64_t* array_shape, double a, double b,
             uint64_t seed, void* stream);

/* -------------------------------------------------------- reduce finalize
 * Combines P partial rows (part_val[P][n], accumulator dtype acc_dtype, and
 * for ARGMIN/ARGMAX part_idx[P][n] int64) into out[n] of out_dtype
 * (for ARG* ops out is int64 indices and out_val may receive the values).
 * Partials are combined in index order p = 0..P-1, so results are
 * deterministic.  Replaces the per-tile partial merge of
 * _reduce_mapper -> DistArray.update -> tile.merge
 * (spartan/expr/reduce.py:53-67, spartan/array/tile.pyx:201-298).
 */
int spx_reduce_finalize(int op, int acc_dtype, int out_dtype, const void* part_val,
                        const int64_t* part_idx, int64_t P, int64_t n, void* out,
                        void* out_val, void* stream);

/* The two partial sets of a paired column + row sum (a generated 'cols'
 * kernel that also writes per-tile row sums) in one launch; dtype SPX_F32 or
 * SPX_F64 for partials and results alike.  col_part[P][n] -> col_out[n]
 * exactly as spx_reduce_finalize(SPX_OP_SUM, dtype, dtype, ...) folds it
 * (bit-identical).  row_part[CT][R] -> row_out[R], folded in ct order in an
 * fp64 accumulator and rounded once to dtype.
 */
int spx_reduce_finalize_pair(int dtype, const void* col_part, int64_t P, int64_t n, void* col_out,
                             const void* row_part, int64_t CT, int64_t R, void* row_out, void* stream);

/* ------------------------------------------------------------------ merge
 * dst[region] = reducer(dst[region], src) with the reference's mask rule:
 * elements whose mask byte is 0 are replaced (first write), others reduced;
 * afterwards the region's mask bytes are 1.  With full_tile_fastpath != 0 and
 * the region equal to the whole tile, the reference's fast path is used: the
 * whole tile is reduced iff mask[0] is set, else replaced
 * (spartan/array/tile.pyx:264-284).  mask may be NULL (treated as all-set
 * for op != REPLACE).  src has src_dtype and is dense with region_shape.
 */
int spx_merge(int op, int dtype, void* dst, uint8_t* mask, int ndim,
              const int64_t* dst_shape, const int64_t* region_ul,
              const int64_t* region_shape, const void* src, int src_dtype,
              int full_tile_fastpath, void* stream);

/* ------------------------------------------------------------ copy region
 * Strided N-d copy with dtype conversion: dst[dst_ul + i] = src[src_ul + i]
 * for i in copy_shape.  Replaces the stitch loop of DistArrayImpl.fetch
 * (spartan/array/distarray.py:315-365) and Tile.get (tile.pyx:69-114).
 */
int spx_copy_region(int dst_dtype, void* dst, const int64_t* dst_shape,
                    const int64_t* dst_ul, int src_dtype, const void* src,
                    const int64_t* src_shape, const int64_t* src_ul, int ndim,
                    const int64_t* copy_shape, void* stream);

/* ------------------------------------------------------------------- gemm
 * C[M,N] = alpha * A[M,K] @ B[K,N] + beta * C, row-major with leading
 * dimensions lda/ldb/ldc, dtype F32 (v_mfma_f32_32x32x2_f32) or F64
 * (v_mfma_f64_16x16x4_f64).  Replaces tiles[0].dot(tiles[1]) in
 * dot_map2_mapper (spartan/expr/dot.py:195-212), dot_outer_mapper (:217-233)
 * and dot_map2_np_mapper (:172-187).
 * Memory: C must be coarse-grained device memory (hipMalloc / a torch CUDA
 * tensor).  The fp32 kernel flushes its accumulators into C every 512
 * K-tiles (fp32 chains of <= 4096 MFMA steps at any K): with K > 8192, or
 * with beta != 0, C is updated by no-return fp32 atomic adds, which are not
 * reliably performed on fine-grained or host-coherent allocations.  One wave
 * owns each element of C, so the adds land in program order (deterministic).
 */
int spx_gemm(int dtype, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
             const void* B, int64_t ldb, void* C, int64_t ldc, double alpha,
             double beta, void* stream);

/* spx_gemm_plan (pure host): the route spx_gemm takes for these arguments --
 * both call the one selection function.  A and B are looked at for their
 * address bits only (16-byte alignment) and never dereferenced, so any
 * non-null value will do.  Any output may be NULL.
 *   kernel   SPX_GEMM_*: which kernel runs (NONE: M == 0 or N == 0, no launch)
 *   aligned  1: the instantiation without bounds checks (whole block tiles,
 *            16-byte aligned operands and rows); 0: the bounds-checked one
 *   bm, bn, bk  the block tile and the K-tile
 *   flush_k  the K distance after which the kernel's accumulators go into C
 *            (fp32: 512 K-tiles; F64_P3: one launch per 8192 of K); 0 for the
 *            kernels whose one chain spans any K
 * Returns the argument errors of spx_gemm (those about C and ldc aside).
 * The choice between the two- and the three-stage kernels follows
 * SPX_GEMM_P3 in the environment (read once per process): 0 never, 1 (the
 * default) fp32 only, 2 fp64 too. */
#define SPX_GEMM_NONE 0
#define SPX_GEMM_INT 1        /* k_gemm_int, 16x16 tiles                       */
#define SPX_GEMM_F32_SMALL 2  /* two-stage 128x128x16, < 512 256x256 tiles     */
#define SPX_GEMM_F32_BIG 3    /* two-stage 256x128x16                          */
#define SPX_GEMM_F32_P3 4     /* three-stage 256x256x16, aligned products only */
#define SPX_GEMM_F64 5        /* two-stage 128x128x16                          */
#define SPX_GEMM_F64_P3 6     /* three-stage 128x128x16 (experimental)         */
int spx_gemm_plan(int dtype, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
                  const void* B, int64_t ldb, int64_t* kernel, int64_t* aligned,
                  int64_t* bm, int64_t* bn, int64_t* bk, int64_t* flush_k);

/* ------------------------------------------------- arg-reduction combine
 * Element-wise combine of R (value, index) partial sets, e.g. gathered from
 * all ranks: out_idx[n] / out_val[n] = best over r of (vals[r][n], idx[r][n]);
 * smaller (ARGMIN) / larger (ARGMAX) value wins, ties go to the smaller
 * index (first occurrence), matching the sentinel-min of _arg_mapper
 * (spartan/expr/builtins.py:610-666).
 */
int spx_argreduce_combine(int op, int dtype, const void* vals, const int64_t* idx,
                          int64_t R, int64_t n, void* out_val, int64_t* out_idx,
                          void* stream);

/* ---------------------------------------------------------------- k-means
 * Assignment step of KMeans.fit (spartan/examples/sklearn/cluster/k_means_.py:
 * 126-128): labels[p] = first argmin over c of cdist(P[p], C[c]) computed
 * exactly as scipy's fp64 euclidean cdist (sequential sum of squared
 * differences, separately rounded, then sqrt) -> bit-exact labels.  points
 * F32/F64 (N, D) with row stride ldp; centers fp64 (K, D).
 * With a workspace (>= spx_kmeans_assign_workspace(dtype, N, D, K) bytes) and
 * mindist == NULL, MFMA passes first certify the points whose nearest centre
 * is separated from the runner-up by more than a rigorous error bound (fp32
 * points, K <= 256, D % 64 == 0: an fp16 screen over every point, then a
 * bf16x3 pass over the points it leaves undecided; other shapes: one fp32
 * MFMA pass); only the remaining points run the exact-order kernel.  The
 * labels are the same bits either way.  With mindist != NULL (receives the fp64 distance)
 * or workspace == NULL every point takes the exact-order kernel.
 * dist_dtype SPX_F64: argmin of the fp64 distances; SPX_F32: argmin of the
 * distances rounded to fp32, first index on equal rounded values -- the
 * outer product's target is fp32 when the points are (map2 / outer dtype
 * None -> arrays[0].dtype, k_means_.py:126-127), and the reference rounds the
 * cdist values into it before argmin.  The certified gap then also covers
 * the rounding (exact distances more than 2 fp32 ulps apart).
 */
int64_t spx_kmeans_assign_workspace(int dtype, int64_t N, int64_t D, int64_t K);
int spx_kmeans_assign(int dtype, int64_t N, int64_t D, int64_t K, const void* points, int64_t ldp,
                      const double* centers, int64_t* labels, double* mindist, void* workspace,
                      size_t workspace_bytes, int dist_dtype, void* stream);
/* Per-centre sums (fp64, K x D) and counts (K) of the points carrying each
 * label (labels outside [0, K) are skipped), ADDED into sums/counts (which are
 * overwritten instead when zero_first != 0): replaces kmeans_center_mapper /
 * kmeans_count_mapper (k_means_.py:61-89).  No float atomics: per-block fp64
 * partials go to the caller's workspace and are summed in a fixed order, so
 * the result is deterministic.  workspace_bytes must be at least
 * spx_kmeans_accumulate_workspace(dtype, N, D, K) (< 0 on bad arguments). */
int64_t spx_kmeans_accumulate_workspace(int dtype, int64_t N, int64_t D, int64_t K);
int spx_kmeans_accumulate(int dtype, int64_t N, int64_t D, int64_t K, const void* points, int64_t ldp,
                          const int64_t* labels, double* sums, uint64_t* counts, int zero_first,
                          void* workspace, size_t workspace_bytes, void* stream);
/* One k-means iteration's device work, fused: spx_kmeans_assign (labels, bit
 * for bit the same) followed by spx_kmeans_accumulate (counts exact, sums
 * deterministic) -- the argmin of outer((X, C), kmeans_dist_mapper) plus
 * kmeans_count_mapper / kmeans_center_mapper of one KMeans.fit iteration
 * (k_means_.py:126-136).  For fp32 points with K <= 256 and D in {64, 128}
 * the decided rows are labelled AND accumulated in one pass over the points
 * (k_kmeans_pp); their sums run in fp32 per block and window of 504 32-row
 * units -- one centre's chain is as long as that centre's rows in the window,
 * ~63 on average at K = 256 on uniform data and up to 16128 when one centre
 * takes every row (K = 1 or 2, skewed data) -- and the window sums are added
 * in fp64 in a fixed order.  A row the screen cannot decide is added
 * PROVISIONALLY to its screen-best centre p when its centred norm |x - mu| is
 * at most 4 (max_c |c - mu| + |mu|), and moved in fp64 afterwards if its final
 * label differs (farther rows are gathered in fp64 instead).  So a window
 * chain holds the centre's own rows plus at most a few such movers of the
 * data's own scale, and its a-priori bound is that of an fp32 sum of <= 16128
 * terms of that scale (<= 16128 u (sum |x| + |movers|), u = 2^-24); the
 * reference's own kmeans_center_mapper sums ALL of a centre's rows in one fp32
 * chain (k_means_.py:67-89).  Measured within 1e-5 of sum |x| in every test,
 * including the long-chain cases and far undecided outliers.
 * Other shapes run the two calls.  workspace_bytes >=
 * spx_kmeans_step_workspace(dtype, N, D, K). */
int64_t spx_kmeans_step_workspace(int dtype, int64_t N, int64_t D, int64_t K);
/* Timing aid (bench / profiling): spx_kmeans_timing(1) makes every later
 * fused spx_kmeans_step record HIP events on its stream around its one-pass
 * kernel and around the whole step (up to 256 calls; 0 turns it off and frees
 * the events).  spx_kmeans_times waits for the recorded calls and writes their
 * kernel / whole-step device times (ms) in call order, clears the record and
 * returns how many it wrote (< 0 on error). */
int spx_kmeans_timing(int enable);
int spx_kmeans_times(double* fused_ms, double* step_ms, int max);
int spx_kmeans_step(int dtype, int64_t N, int64_t D, int64_t K, const void* points, int64_t ldp,
                    const double* centers, int64_t* labels, double* sums, uint64_t* counts, int zero_first,
                    void* workspace, size_t workspace_bytes, int dist_dtype, void* stream);

/* Full distance matrix out[p * ldo + c] = cdist(points, centers)[p, c] in
 * the exact order above, rounded once to out_dtype (F32/F64): the
 * materialised outer((X, C), (0, 0), kmeans_dist_mapper) (k_means_.py:52-58,
 * outer.py:14-61).  points F32/F64 (N, D) row stride ldp; centers fp64. */
int spx_cdist(int dtype, int out_dtype, int64_t N, int64_t D, int64_t K, const void* points, int64_t ldp,
              const double* centers, void* out, int64_t ldo, void* stream);
/* counts[k] (+)= number of labels equal to k (labels outside [0, K)
 * skipped; overwritten when zero_first != 0): np.bincount(labels,
 * minlength=K) of kmeans_count_mapper (k_means_.py:61-64).  Exact. */
int spx_bincount(const int64_t* labels, int64_t N, int64_t K, uint64_t* counts, int zero_first, void* stream);

/* ------------------------------------------------------------ prefix scan
 * np.cumsum along one axis of a tile: the per-tile scan_fn of _scan_mapper and
 * the per-tile reduce_fn of _scan_reduce_mapper (spartan/expr/scan.py:24-64).
 * `in` is a dense row-major block viewed as (outer, n, inner); the scan runs
 * along n for each of the outer * inner lines.  Additive since ABI 3.
 * Result dtype as np.cumsum: BOOL / I32 / I64 in -> I64 out, F32 -> F32,
 * F64 -> F64.  The accumulator is 64-bit integer (unsigned arithmetic, so
 * wrap-around is defined) for the integer inputs and fp64 for both float
 * types: an fp32 scan is accumulated in fp64 and rounded once on store.
 * carry / totals are dense (outer, inner) arrays in the accumulator dtype
 * (I64 / F64), so bases are never rounded between tiles or ranks.
 *   carry   NULL, or added to every element of its line;
 *   totals  NULL, or receives each line's inclusive total WITHOUT the carry;
 *   out     NULL for a totals-only pass (out and totals both NULL: SPX_EINVAL);
 *   exclusive != 0: out[i] = carry + sum of in[j], j < i.
 * Lines that are long and too few to fill the GPU are cut into chunks over
 * three launches (chunk totals, their scan, the chunk scans): the input is
 * then read twice, and workspace_bytes must be at least
 * spx_scan_workspace(in_dtype, outer, n, inner) (0 for the single-pass
 * geometry; < 0 on bad arguments).  No launch has one workgroup wait for
 * another.  Fixed addition order, no atomics: the same input and geometry
 * give the same bits.  Arguments are checked before any device work. */
int64_t spx_scan_workspace(int in_dtype, int64_t outer, int64_t n, int64_t inner);
int spx_scan(int in_dtype, const void* in, void* out, int64_t outer, int64_t n, int64_t inner,
             const void* carry, void* totals, int exclusive, void* workspace, size_t workspace_bytes,
             void* stream);

/* ---------------------------------------------------------- sort / argsort
 * np.sort / np.argsort(kind='stable') along one axis of a tile: the per-tile
 * _sort_mapper / _argsort_mapper of spartan/expr/sort.py:78-91.  `in` is a
 * dense row-major block viewed as (outer, n, inner), as in spx_scan; each of
 * the outer * inner lines is sorted ascending along n.  Additive since ABI 3.
 *   out_vals  NULL, or in's dtype: the sorted values;
 *   out_idx   NULL, or int64: the positions 0..n-1 within the line (argsort);
 *             both NULL: SPX_EINVAL.  `in` may not alias an output.
 * dtypes BOOL / I32 / I64 / F32 / F64.  The sort is STABLE and keys compare
 * as NumPy compares them: integers signed, bool 0 < 1, -0.0 == +0.0 (zeros tie
 * and keep input order), every NaN ties with every other NaN and sorts after
 * +inf.  So out_idx is np.argsort(x, axis=1, kind='stable') bit for bit and
 * in[out_idx] along the line is out_vals.  out_vals is a permutation of the
 * line's bit patterns (the signs of zeros included) except that NaNs, which
 * come last, have their sign and payload canonicalised.
 * Lines of n <= 2048 are sorted in LDS (one read, one write, no workspace);
 * longer lines take least-significant-digit radix passes of 8 bits (1 / 4 /
 * 8 passes for BOOL / 32-bit / 64-bit keys), three launches each (per-tile
 * digit counts, their exclusive scan, a stable scatter), ping-ponging between
 * two buffers in the workspace; strided lines (inner > 1) are transposed into
 * the workspace before the passes and back into the outputs after them (two
 * more passes over the data).  No launch has one workgroup wait for another;
 * no float atomics; the same input and geometry give the same bits.
 * workspace_bytes must be at least spx_sort_workspace(dtype, outer, n, inner,
 * out_idx != NULL) (0 for the LDS path; < 0 on bad arguments).  Arguments are
 * checked before any device work: SPX_EINVAL for null / negative arguments,
 * an unknown dtype or a short workspace, SPX_ENOTSUP for n >= 2^31; n == 0 or
 * zero lines is SPX_OK with no launch.
 * spx_sort_plan returns the number of radix passes the geometry takes (0: the
 * LDS path; < 0 on bad arguments) and writes the longest LDS-path line and
 * the radix tile length (either pointer may be NULL). */
int64_t spx_sort_workspace(int dtype, int64_t outer, int64_t n, int64_t inner, int want_idx);
int spx_sort(int dtype, const void* in, void* out_vals, int64_t* out_idx, int64_t outer, int64_t n,
             int64_t inner, void* workspace, size_t workspace_bytes, void* stream);
int spx_sort_plan(int dtype, int64_t outer, int64_t n, int64_t inner, int64_t* lds_max, int64_t* tile);

/* ------------------------------------------------------------ topk / argtopk
 * The first k elements of each line's stable order, without sorting the line.
 * `in` is a dense row-major block viewed as (outer, n, inner) as in spx_sort;
 * the outputs are dense (outer, k, inner).  Additive since ABI 3.
 *   largest == 0: positions np.argsort(x, kind='stable')[:k] -- spx_sort's
 *     order (integers signed, bool 0 < 1, -0.0 == +0.0, NaNs tie and come after
 *     +inf), equal keys lower position first;
 *   largest != 0: descending by value, equal keys lower position first, NaNs
 *     still last: np.argsort(-x, kind='stable')[:k] for floats and
 *     np.argsort(~x, kind='stable')[:k] for BOOL / I32 / I64;
 *   out_vals  NULL, or in's dtype: the selected elements' bit patterns;
 *   out_idx   NULL, or int64: the positions within the line, or, with in_idx
 *             (int64, in's shape; may be NULL), in_idx at those positions --
 *             ties are still broken by position.  Both outputs NULL: SPX_EINVAL.
 * 1 <= k <= n, k at most the limit the plan call reports through kmax (2048:
 * the selected candidates of a line are ordered by one LDS sort); a larger k is
 * SPX_ENOTSUP, as is n >= 2^31.  Lines of n <= 2048 are sorted in LDS and only
 * the first k stored (no workspace).  Longer lines take a most-significant-
 * digit radix select of 8 bits a pass over the order keys (three launches a
 * pass: per-chunk digit counts of the keys matching the prefix, one workgroup
 * per line picks the digit of the k-th key, one wave per chunk counts the keys
 * now known to precede it), one stable compaction
 * pass that writes the k candidates in position order and one LDS sort of the
 * candidates: the line is read (key bytes + 1) times and never written, and
 * strided lines (inner > 1) are indexed with their stride.  No launch has one
 * workgroup wait for another; no float atomics; the same input and geometry
 * give the same bits.  workspace_bytes must be at least the workspace call's
 * answer for (dtype, outer, n, inner, k, out_idx != NULL) (0 for the LDS path;
 * < 0 on bad arguments).  Arguments are checked before any device work:
 * SPX_EINVAL for null / negative arguments, an unknown dtype, k < 1, k > n or a
 * short workspace; zero lines is SPX_OK with no launch.  The plan call returns
 * the number of select passes (0: the LDS path; < 0 on bad arguments) and
 * writes the k limit and the chunk of a line one workgroup counts (either
 * pointer may be NULL). */
int64_t spx_topk_workspace(int dtype, int64_t outer, int64_t n, int64_t inner, int64_t k, int want_idx);
int spx_topk(int dtype, const void* in, const int64_t* in_idx, void* out_vals, int64_t* out_idx, int64_t outer,
             int64_t n, int64_t inner, int64_t k, int largest, void* workspace, size_t workspace_bytes,
             void* stream);
int spx_topk_plan(int dtype, int64_t outer, int64_t n, int64_t inner, int64_t k, int64_t* kmax, int64_t* chunk);

/* -------------------------------------------------------- nearest neighbours
 * The brute-force search of NearestNeighbors.kneighbors
 * (spartan/examples/sklearn/neighbors/unsupervised.py), fused: distances and
 * selection in one kernel, the (Q, N) matrix never written.  points F32 / F64
 * (N, D) with row stride ldp; queries fp64, dense (Q, D).  s[i, j] is the fp64
 * sum over d = 0..D-1, in that order, of (queries[i, d] - (double)points[j,
 * d])^2, every difference, square and add rounded separately and the
 * accumulator starting at +0.0: the value whose sqrt the distance-matrix call
 * above stores.  The neighbours of query i are the first k of the order (s[i,
 * j], j) ascending, NaN sums after +inf.  out_s (Q, k) fp64 receives the sums
 * (not their roots; NaNs canonical), out_idx (Q, k) int64 index_base + j.
 * 1 <= k <= N, k at most the limit the plan call reports through kmax (128); a
 * larger k is SPX_ENOTSUP, as is N >= 2^31; any D >= 1.  The points are cut
 * into ranges over the grid's second dimension so that a few queries still
 * fill the GPU; each (64-query tile, range) leaves its k best in the workspace
 * and the selection kernels above pick per query among the ranges' lists.  The
 * composite (s, j) is a total order, so the result does not depend on the
 * ranges or on the order in which candidates met.  No workgroup waits for
 * another; no float atomics; same input, same bits.  workspace_bytes must be at
 * least the workspace call's answer (< 0 on bad arguments); SPX_EINVAL for null
 * pointers, negative sizes, ldp < D, k < 1, k > N or a short workspace, checked
 * before any device work; Q == 0 is SPX_OK with no launch.  The plan call
 * returns the number of point ranges (< 0 on bad arguments) and writes the k
 * limit and the range length (either pointer may be NULL). */
int64_t spx_knn_workspace(int dtype, int64_t Q, int64_t N, int64_t D, int64_t k);
int spx_knn(int dtype, int64_t Q, int64_t N, int64_t D, int64_t k, const void* points, int64_t ldp,
            const double* queries, int64_t index_base, double* out_s, int64_t* out_idx, void* workspace,
            size_t workspace_bytes, void* stream);
int spx_knn_plan(int dtype, int64_t Q, int64_t N, int64_t D, int64_t k, int64_t* kmax, int64_t* chunk);

/* ---------------------------------------------------------- take / compress
 * Indexing a tile by an index array or a mask: np.take(a, idx, axis) -- the
 * integer path of spartan/expr/filter.py:50-76 -- and np.compress / a[mask].
 * Blocks are dense row-major, viewed as (outer, n, inner) as in spx_scan.
 * Values move as bit patterns of their element size (1 / 4 / 8 bytes; `dtype`
 * only selects the size); no atomics; the same input gives the same bits.
 * Arguments are checked before any device work: SPX_EINVAL for null or
 * negative arguments, an unknown dtype or a short workspace; empty work is
 * SPX_OK with no launch.  Additive since ABI 3.
 *
 * spx_take: `src` is the block (outer, n_local, inner) holding rows [lo, lo +
 * n_local) of an axis of length n_total; idx holds m indices (idx_dtype I32 /
 * I64).  For j < m, r = idx[j] (+ n_total when negative):
 *   r outside [0, n_total): *err = 1 (a device word the call clears first),
 *     nothing is read or written for j;
 *   r outside [lo, lo + n_local): out row j is left untouched;
 *   otherwise out[o * out_outer_stride + j * out_row_stride + c] =
 *     src[o, r - lo, c] (strides in elements, c < inner contiguous).
 * The range test comes before any address is formed.  Rows shorter than 64
 * units (a unit: 16 bytes where the row bytes, both strides and both pointers
 * are multiples of 16, one element otherwise) take one lane per unit, longer
 * rows a wave (from 2048 units a workgroup) per four rows.
 *
 * spx_compact_count / spx_compact: `mask` is n bytes, any nonzero byte selects.
 * spx_compact_count counts the selected bytes per tile of a fixed number of
 * mask bytes into an int64 table in the workspace, scans the table exclusively
 * in place and writes the total to the DEVICE word `total` (n == 0: the word is
cleared by a memset, no kernel is launched).  spx_compact reads
 * the mask again, ranks the selected positions of a tile (wave ballots and
 * popcounts, wave counts met in LDS) and writes out[o, base[tile] + rank, :] =
 * in[o, j, :]; `out` is the dense block (outer, count, inner) and `count` must
 * be the total (positions at or past `count` are not written).  `workspace` is
 * the one spx_compact_count filled: spx_compact_workspace(n) bytes (0 for n ==
 * 0, < 0 on a bad n), 8-byte aligned; its first 8 * ceil(n / tile) bytes are
 * the table.  No launch has one workgroup wait for another. */
int spx_take(int dtype, int idx_dtype, const void* src, const void* idx, void* out, int64_t outer,
             int64_t n_total, int64_t lo, int64_t n_local, int64_t m, int64_t inner, int64_t out_outer_stride,
             int64_t out_row_stride, int32_t* err, void* stream);
int64_t spx_compact_workspace(int64_t n);
int spx_compact_count(const void* mask, int64_t n, int64_t* total, void* workspace, size_t bytes, void* stream);
int spx_compact(int dtype, const void* in, const void* mask, void* out, int64_t outer, int64_t n, int64_t inner,
                int64_t count, const void* workspace, size_t bytes, void* stream);

/* ------------------------------------------------------ stencil / maxpool
 * The convnet pair of spartan/expr/stencil.py on contiguous blocks.
 * spx_stencil replaces _convolve (stencil.py:27-43), a Parakeet imap of the
 * scalar loop: images (N, C, W, H), filters (F, C, fw, fh), out (N, F, W, H),
 *   out[n, f, x, y] = sum over c, i, j with x + i < W and y + j < H of
 *                     images[n, c, x + i, y + j] * filters[f, c, i, j]
 * -- cross-correlation anchored at the top-left, taps past the bottom / right
 * edge dropped.  Per image it is one MFMA product with M = F, N = W H, K = C fw
 * fh whose B operand (the shifted, clipped image) is formed while staging into
 * LDS and never written to memory; float32 and float64 only; one accumulation
 * chain per element.  spx_stencil_plan returns the block tile (rows of F,
 * columns of W H, K-tile) of a dtype; any of the three pointers may be NULL.
 * spx_maxpool is the loop _maxpool has in its commented-out lines
 * (stencil.py:58-67; the live body is a stub that returns a constant array):
 * in (NC, W, H), out (NC, ceil(W / stride), ceil(H / stride)),
 *   out[r, p, q] = max over i, j < pool with p stride + i < W and q stride + j < H
 *                  of in[r, p stride + i, q stride + j]
 * for the five dtypes (bool as bytes); every window holds its first element,
 * so there is no fill value; NaN propagates as in np.maximum.  Both: N (NC)
 * == 0 launches nothing; SPX_EINVAL for a bad dtype, a null pointer or a
 * non-positive extent, SPX_ENOTSUP where an extent overflows the kernel's
 * indices (stencil: (C + 16) W H, F W H, F C fw fh and (fw + 1) H must stay
 * below 2^31).  No atomics; no workgroup waits for another. */
int spx_stencil_plan(int dtype, int64_t* bm, int64_t* bn, int64_t* bk);
int spx_stencil(int dtype, const void* images, const void* filters, void* out, int64_t N, int64_t C, int64_t W,
                int64_t H, int64_t F, int64_t fw, int64_t fh, void* stream);
int spx_maxpool(int dtype, const void* in, void* out, int64_t NC, int64_t W, int64_t H, int64_t pool,
                int64_t stride, void* stream);

/* ------------------------------------------------- cholesky / triangular solve
 * Dense linear algebra on one tile: the three mappers of
 * spartan/examples/cholesky.py (scipy's dpotrf, dtrtrs / dtrsm, dsyrk / dgemm).
 * float32 and float64 only (another dtype: SPX_ENOTSUP); row-major with leading
 * dimensions in elements; asynchronous on the stream.  Arguments are checked
 * before any device work: SPX_EINVAL for a null pointer, a negative size, a
 * leading dimension below the row length or a short workspace, SPX_ENOTSUP for
 * an extent whose tile count reaches 2^31; empty work is SPX_OK with no launch.
 * No workgroup waits for another, no float atomics, the same input and
 * geometry give the same bits.  Additive since ABI 3.
 *
 * The factorization: L = the lower Cholesky factor of the n x n matrix A.  Only
 * A's lower triangle (i >= j) is read; L's strict upper triangle is written as
 * +0.0; L may be A (then lda == ldl).  Blocked right-looking at two levels
 * (the plan call reports the diagonal block nb, factored by one workgroup in
 * LDS, and the outer panel nb_outer, the K of the trailing update).  `info` is a
 * device int32 word the call clears first: it stays 0 on success and otherwise
 * receives the 1-based order of the first leading minor whose pivot is <= 0 or
 * NaN (LAPACK's info); the host never reads it inside the call, every launch
 * still completes after a failed pivot and the rest of L is then unspecified.
 * The workspace call's answer (0 here: the work is done in place on L; < 0 on
 * bad arguments) is the least workspace_bytes.
 *
 * The triangular solve, in place on B (m x n), with a lower-triangular,
 * non-unit L: side LEFT solves op(L) X = B (L m x m), side RIGHT X op(L) = B
 * (L n x n); op N or T.  RIGHT/T and RIGHT/N have kernels of their own
 * (diagonal blocks by substitution with true divisions -- no inverse, no
 * reciprocal --, off-diagonal blocks on MFMA); the LEFT forms run them on a
 * transposed copy of B in the workspace (m n elements).  No singularity check:
 * a zero diagonal gives IEEE inf / NaN.
 *
 * The update: C[M,N] -= A[M,K] B[N,K]^T on v_mfma_f32_32x32x2_f32 /
 * v_mfma_f64_16x16x4_f64, both operands read along their rows, one
 * accumulation chain per element, C read and written once.  lower != 0 (needs
 * M == N, C's diagonal on the tile diagonal): tiles strictly above the
 * diagonal are not launched and diagonal tiles touch only i >= j. */
#define SPX_SIDE_LEFT 0
#define SPX_SIDE_RIGHT 1
#define SPX_TRANS_N 0
#define SPX_TRANS_T 1
int spx_potrf_plan(int dtype, int64_t* nb, int64_t* nb_outer);
int64_t spx_potrf_workspace(int dtype, int64_t n);
int spx_potrf(int dtype, int64_t n, const void* A, int64_t lda, void* L, int64_t ldl, int32_t* info,
              void* workspace, size_t workspace_bytes, void* stream);
int64_t spx_trsm_workspace(int dtype, int side, int64_t m, int64_t n);
int spx_trsm(int dtype, int side, int op, int64_t m, int64_t n, const void* L, int64_t ldl, void* B, int64_t ldb,
             void* workspace, size_t workspace_bytes, void* stream);
int spx_syrk(int dtype, int lower, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
             int64_t ldb, void* C, int64_t ldc, void* stream);

/* ------------------------------------------------------------- qr (TSQR)
 * The reduced QR factorization A = Q R of a tall or square m x n matrix
 * (m >= n) by communication-avoiding Householder QR: the thin QR that
 * spartan/examples/ssvd/qr.py obtains from a Cholesky factor of A^T A, here
 * backward stable for any conditioning and any rank.  float32 and float64 only
 * (another dtype: SPX_ENOTSUP); row-major with leading dimensions in elements;
 * asynchronous on the stream.
 *
 * The plan call returns SPX_OK and writes the column limit *nmax of the dtype
 * (128 for float32, 64 for float64) and *rows = r(dtype, n), the rows one
 * workgroup factors in LDS (a multiple of 64, at least 2 n; 0 where n > nmax);
 * either pointer may be NULL.  The workspace call answers the bytes spx_geqr
 * needs for (m, n) -- it grows monotonically in m and is about m n elements --
 * or < 0 on bad arguments (m < n and n > nmax included).
 *
 * spx_geqr reads A once and never writes it: ceil(m / r) workgroups factor one
 * block of r rows each, their n x n triangles are stacked and factored by the
 * same kernel, and so on until one block remains.  R (n x n) receives that
 * block's triangle with +0.0 strictly below the diagonal and its rows scaled so
 * that diag(R) >= 0; the workspace receives every block's reflectors and taus
 * and the sign matrix D.  spx_orgqr forms Q (m x n) = Q_0 D C from them, C the
 * n x n seed (NULL: the identity; C is read only), so that A = Q R for C = I;
 * it uses the workspace's stack regions as scratch for the tree's inner levels
 * (which is why the workspace is not const) and leaves the reflectors intact:
 * it may be called again with another seed.  Bytes beyond column n of any row
 * of A, R, C and Q are neither read nor written.  A zero column below the
 * diagonal gives tau = 0; column norms are accumulated in double (float data)
 * or scaled by a power of two (double data).  No atomics, no workgroup waits
 * for another, the same input and geometry give the same bits.
 *
 * Arguments are checked before any device work: SPX_EINVAL for a null pointer,
 * a negative size, m < n, a leading dimension below n or a short workspace,
 * SPX_ENOTSUP for n > nmax; m == 0 or n == 0 is SPX_OK with no launch.
 * Additive since ABI 3. */
int spx_geqr_plan(int dtype, int64_t n, int64_t* nmax, int64_t* rows);
int64_t spx_geqr_workspace(int dtype, int64_t m, int64_t n);
int spx_geqr(int dtype, int64_t m, int64_t n, const void* A, int64_t lda, void* R, int64_t ldr, void* workspace,
             size_t workspace_bytes, void* stream);
int spx_orgqr(int dtype, int64_t m, int64_t n, void* workspace, size_t workspace_bytes, const void* C, int64_t ldc,
              void* Q, int64_t ldq, void* stream);

/* ------------------------------------------- symmetric eigen-solver (Jacobi)
 * All eigenvalues and eigenvectors of `batch` symmetric n x n matrices, what
 * np.linalg.eigh computes for an (..., n, n) array, by the parallel cyclic
 * Jacobi method: one workgroup per matrix, which never leaves LDS, the grid
 * over the batch.  float32 and float64 only (another dtype: SPX_ENOTSUP);
 * asynchronous on the stream; no workspace.
 *
 * The plan call returns SPX_OK and writes the size limit *nmax of the dtype
 * (128 for float32, 96 for float64: A and V, n columns of n + 1 each, and the
 * round's table fit the 160 KiB one workgroup may declare) and *sweep_max (64);
 * either pointer may be NULL.
 *
 * Matrix b is A + b stride_a, row-major with leading dimension lda >= n; only
 * the triangle named by uplo (0: 'L', 1: 'U') is read -- the other one may hold
 * anything, NaN included -- and A is never written.  W + b stride_w receives the
 * n eigenvalues in ascending order, V + b stride_v (n x n, leading dimension
 * ldv) the eigenvectors as columns in the same order, each with its entry of
 * largest magnitude (the first on a tie) positive.  info[b] is the number of
 * sweeps used (>= 0; 0 for the zero matrix and for n = 1), or -1 when matrix b
 * did not converge within sweep_max sweeps or its triangle holds a non-finite
 * value: W and V of that matrix are then filled with NaN and the other
 * matrices of the batch are not affected.  Bytes beyond column n of any row of
 * A and V, and beyond entry n of W, are neither read nor written.
 *
 * The matrix is scaled by the power of two of its largest magnitude (exact);
 * a pair is rotated while |a_pq| > u ||A||_F / n (u the unit roundoff), so that
 * off(A)_F < u ||A||_F at convergence; a sweep is the m - 1 rounds of a
 * round-robin ordering over m = n + (n & 1) indices.  The workgroup size
 * depends on n alone and there are no atomics: a matrix gives the same bits
 * wherever it stands in a batch and whatever the batch size.
 *
 * Arguments are checked before any device work: SPX_EINVAL for a null pointer,
 * a negative size, an uplo other than 0 / 1, a leading dimension below n, a
 * negative stride_a or (batch > 1) output strides that let two matrices
 * overlap; SPX_ENOTSUP for n > nmax or batch >= 2^31; batch == 0 or n == 0 is
 * SPX_OK with no launch.  Additive since ABI 3. */
int spx_syevj_plan(int dtype, int64_t* nmax, int64_t* sweep_max);
int spx_syevj(int dtype, int uplo, int64_t batch, int64_t n, const void* A, int64_t lda, int64_t stride_a, void* W,
              int64_t stride_w, void* V, int64_t ldv, int64_t stride_v, int32_t* info, void* stream);

/* ------------------------------------------- dense SVD (one-sided Jacobi)
 * The reduced singular value decomposition A = U diag(S) Vt of `batch`
 * row-major m x n matrices with m >= n, what np.linalg.svd(full_matrices=False)
 * computes for an (..., m, n) array, by the one-sided (Hestenes) Jacobi method:
 * one workgroup per matrix, which never leaves LDS, the grid over the batch.
 * The method rotates the columns of A itself and never forms A^T A, so small
 * singular values are resolved to high relative accuracy.  float32 and float64
 * only (another dtype: SPX_ENOTSUP); asynchronous on the stream; no workspace,
 * no atomics.
 *
 * The plan call returns SPX_OK and writes the column limit *nmax of the dtype
 * (the largest multiple of 32 for which a square matrix fits: 128 for float32,
 * 96 for float64), the row limit *mmax for n columns (the largest m whose
 * working copy, n columns of m | 1, fits the 160 KiB one workgroup may declare
 * beside V, n columns of n | 1; 0 for n > nmax) and *sweep_max (64); any pointer
 * may be NULL.  The plan describes jobu == 1; with jobu == 0 V is not held and
 * spx_gesvj accepts the correspondingly larger m.
 *
 * Matrix b is A + b stride_a with leading dimension lda >= n; A is read once
 * and never written.  S + b stride_s receives the n singular values, descending
 * and non-negative.  With jobu == 1, U + b stride_u (m x n, leading dimension
 * ldu) receives the left singular vectors as columns and Vt + b stride_vt
 * (n x n, leading dimension ldvt) the right ones as rows, in the same order;
 * with jobu == 0 only S is computed and U and Vt must be NULL.  In every row of
 * Vt the entry of largest magnitude (the first on a tie) is positive; the
 * column of U carries the sign.  For an exactly zero singular value the column
 * of U is exactly zero (LAPACK gesvj's contract: only the columns of nonzero
 * singular values are orthonormal); two equal columns and a zero column of A
 * give such a zero.  A = U diag(S) Vt and Vt Vt^T = I hold regardless.
 * info[b] is the number of sweeps used (>= 0; 0 for the zero matrix and for
 * n = 1), or -1 when matrix b did not converge within sweep_max sweeps or holds
 * a non-finite value: its outputs are then filled with NaN and the other
 * matrices of the batch are not affected.  Bytes beyond column n of any row of
 * A, U and Vt, and beyond entry n of S, are neither read nor written.
 *
 * The matrix is scaled by the power of two of its largest magnitude (exact); a
 * sweep is the m' - 1 rounds of the round-robin ordering of spx_syevj over the
 * m' = n + (n & 1) columns; the pair (p, q) is rotated iff a_pp > 0, a_qq > 0
 * and |a_pq| > sqrt(m) u sqrt(a_pp) sqrt(a_qq), the three dot products formed
 * anew in every round in the data's dtype; a sweep without a rotation ends the
 * iteration.  The workgroup size depends on (m, n) alone: a matrix gives the
 * same bits wherever it stands in a batch and whatever the batch size.
 *
 * Arguments are checked before any device work: SPX_EINVAL for a null pointer
 * (or a non-null U / Vt with jobu == 0), a jobu other than 0 / 1, a negative
 * size, m < n, a leading dimension below n, a negative stride_a or (batch > 1)
 * output strides that let two matrices overlap; SPX_ENOTSUP for n > nmax,
 * m > mmax or batch >= 2^31; batch == 0 or n == 0 is SPX_OK with no launch.
 * Additive since ABI 3. */
int spx_gesvj_plan(int dtype, int64_t n, int64_t* nmax, int64_t* mmax, int64_t* sweep_max);
int spx_gesvj(int dtype, int jobu, int64_t batch, int64_t m, int64_t n, const void* A, int64_t lda, int64_t stride_a,
              void* U, int64_t ldu, int64_t stride_u, void* S, int64_t stride_s, void* Vt, int64_t ldvt,
              int64_t stride_vt, int32_t* info, void* stream);

/* ------------------------------------------------- sparse (CSR) x dense
 * Replaces the scipy.sparse branches of the reference's dot
 * (spartan/expr/dot.py:51, :207-231): a sparse tile times a dense block.
 *
 * spx_csrmm: C = alpha A B + beta C.  A is m x n in CSR -- rowptr (m + 1
 * int64, rowptr[0] == 0, rowptr[m] == nnz), col (nnz int32 in [0, n), sorted
 * within a row), val (nnz float32 / float64) -- B is dense row-major n x p
 * with leading dimension ldb, C is m x p with leading dimension ldc; alpha and
 * beta are cast to dtype.  beta == 0 overwrites C without reading it.  A group
 * of g lanes works on a row (lanes along p first, so B's rows are read
 * coalesced, the rest along the row's nonzeros); rows of more than T nonzeros
 * are cut into chunks of T, one workgroup each, whose partial rows are added in
 * chunk order.  No float atomics: a call's result is bitwise reproducible, and a
 * row's value depends only on its own nonzeros, g and p.  g = 0 takes the g of
 * spx_csrmm_plan for (m, nnz, p); a caller that wants the same bits for every
 * row slab of one matrix passes one g (a power of two in 1 .. 64) to all.
 *
 * The workspace (spx_csrmm_workspace bytes; needed only when nnz > T) starts
 * with the structure analysis -- the list of long rows and of their chunks,
 * a function of rowptr alone -- followed by the call's partial rows.  With
 * prepared == 0 the call builds the analysis (on the stream) before it uses
 * it; with prepared != 0 it trusts what an earlier call for the same rowptr
 * left there.  Neither case synchronises the host.
 *
 * spx_csrmm_plan (pure host): g, T and the rows one 256-thread workgroup
 * covers (256 / g) for a problem.  spx_csrmm_workspace: bytes, or -1 on bad
 * arguments (monotone in m, nnz and p).
 *
 * spx_csr_todense: D (m x n, leading dimension ldd) = A as a dense block:
 * the leading n columns of every row are zero-filled, then every nonzero is
 * stored at its place by a plain vector store (columns within a row are
 * distinct, so no two share a destination).
 *
 * Arguments are checked before any device work: SPX_EINVAL for a dtype code
 * out of range, a negative size, a leading dimension below p (n for
 * todense), a g that is no power of two, a null pointer where it is read
 * (col / val / B only with nnz > 0) or a short workspace; SPX_ENOTSUP for a
 * dtype other than float32 / float64.  m == 0 or p == 0 is SPX_OK with no
 * launch.  Additive since ABI 3. */
int spx_csrmm_plan(int dtype, int64_t m, int64_t nnz, int64_t p, int64_t* g, int64_t* long_row,
                   int64_t* rows_per_block);
int64_t spx_csrmm_workspace(int dtype, int64_t m, int64_t nnz, int64_t p);
int spx_csrmm(int dtype, int64_t m, int64_t n, int64_t p, int64_t nnz, const int64_t* rowptr, const int32_t* col,
              const void* val, const void* B, int64_t ldb, void* C, int64_t ldc, double alpha, double beta,
              int64_t g, void* workspace, size_t workspace_bytes, int prepared, void* stream);
int spx_csr_todense(int dtype, int64_t m, int64_t n, int64_t nnz, const int64_t* rowptr, const int32_t* col,
                    const void* val, void* D, int64_t ldd, void* stream);

/* ------------------------------- sparse transpose helper, ALS row solves
 * spx_csr_rowids: out[k] = r0 + i for every k in [rowptr[i], rowptr[i + 1])
 * -- the global row number of every stored entry of a row slab that starts at
 * row r0, which the transpose sorts along with the values.
 * rowptr is m + 1 int64 with rowptr[m] == nnz, out is nnz int32; every word of
 * out is written once by a plain vector store.  SPX_EINVAL for a negative size
 * or a null pointer, SPX_ENOTSUP for r0 + m above the int32 range; m == 0 or
 * nnz == 0 is SPX_OK with no launch.
 *
 * spx_als_solve: the per-row solve of alternating least squares, replacing the
 * per-row numpy lstsq loop of the reference (spartan/examples/als.py).  A is
 * m x n in CSR as for spx_csrmm, Y is dense row-major n x f with leading
 * dimension ldy, X is m x f with leading dimension ldx.  For every row i, with
 * K_i the stored entries of the row whose value is not zero,
 *
 *   G_i = sum_{k in K_i} y_{col[k]} y_{col[k]}^T + lambda |K_i| I,
 *   b_i = sum_{k in K_i} val[k] y_{col[k]},      X[i, :] = G_i^{-1} b_i
 *
 * by Cholesky and two substitutions.  A row with K_i empty gets zeros.  A row
 * whose factorization meets a pivot that is not positive and finite gets NaN
 * in all f entries, and *info -- a device word the call clears first --
 * counts those rows.  Everything is computed in float64 for both dtypes; the
 * dtype says what is loaded and stored.  One wave owns a row and walks its
 * entries in stored order, so there are no float atomics, a call is bitwise
 * reproducible, and a row's bits depend only on its own entries, Y, f, lambda
 * and dtype -- never on m or on the rows around it.  The columns must lie in
 * [0, n): the kernel does not check them.  X may not alias Y.
 *
 * spx_als_plan (pure host): fmax (64) and the rows one 256-thread workgroup
 * solves for this f (0 where f is outside 1 .. fmax).
 *
 * Arguments are checked before any device work: SPX_EINVAL for a dtype code
 * out of range, a negative size, f < 1, ldy or ldx below f, a lambda that is
 * negative or not finite, a null pointer where it is read (col / val / Y only
 * with nnz > 0) or X == Y; SPX_ENOTSUP for a dtype other than float32 /
 * float64 or f > fmax.  m == 0 is SPX_OK with no launch.  Additive since
 * ABI 3. */
int spx_csr_rowids(int64_t m, int64_t nnz, const int64_t* rowptr, int64_t r0, int32_t* out, void* stream);
int spx_als_plan(int dtype, int64_t f, int64_t* fmax, int64_t* rows_per_block);
int spx_als_solve(int dtype, int64_t m, int64_t n, int64_t f, int64_t nnz, const int64_t* rowptr, const int32_t* col,
                  const void* val, const void* Y, int64_t ldy, double lambda, void* X, int64_t ldx, int32_t* info,
                  void* stream);

/* ------------------------------------------- all-pairs shortest paths
 * Replaces the per-tile Cython Dijkstra of the reference's manifold learner
 * (spartan/examples/util/graph_shortest_path.pyx, called from
 * spartan/examples/sklearn/manifold/isomap.py:11-41) by the blocked
 * Floyd-Warshall recurrence.
 *
 * spx_apsp: G (n x n, row-major, leading dimension ldg) holds edge weights: an
 * off-diagonal G[i][j] is an edge i -> j of that weight iff it is finite and
 * > 0; 0 and +inf both mean "no edge" and the diagonal is ignored.  With
 * directed == 0 the edge between i and j is the smaller of the edges present
 * in G[i][j] and G[j][i].  D (n x n, leading dimension ldd, D != G) receives
 * the length of a shortest path from i to j, D[i][i] = 0, and `unreachable`
 * cast to dtype where there is no path.  *info -- a device word the call
 * clears first -- is 0, or -1 when any entry of G (the diagonal included) is
 * negative, -inf or NaN; D is then unspecified, and nothing faults or loops.
 * G is never written; bytes beyond column n of a row are neither read nor
 * written.
 *
 * The matrix is cut into pivot blocks of edge b (spx_apsp_plan); per block
 * one launch closes the diagonal tile, one updates the block row and block
 * column, one updates every other tile by a (min, +) tile product.  All
 * launches are ordered on `stream`; no host synchronisation, no graph
 * capture, no atomics: a call's result is bitwise reproducible.  When every
 * path sum is exact in dtype, the result is the exact one.
 *
 * Arguments are checked before any device work: SPX_EINVAL for a dtype code
 * out of range, a negative n, an `unreachable` that is negative or NaN, a null
 * pointer, a leading dimension below n or D == G; SPX_ENOTSUP for a dtype
 * other than float32 / float64 or n > 2097120.  n == 0 is SPX_OK with no
 * launch.  Additive since ABI 3. */
int spx_apsp_plan(int dtype, int64_t* tile);
int spx_apsp(int dtype, int directed, int64_t n, const void* G, int64_t ldg, void* D, int64_t ldd, double unreachable,
             int32_t* info, void* stream);

/* ------------------------------------------------- fuzzy k-means step
 * Replaces the expression graph of the reference's soft clustering driver
 * (spartan/examples/fuzzy_kmeans.py), whose (n, k, d) and (n, k, k) broadcasts
 * never fit, by one pass over the points.
 *
 * spx_fuzzy_step: points is N x D row-major with leading dimension ldp, in
 * dtype (float32 / float64); centers is K x D float64, contiguous.  Per row i,
 *
 *   d_ij = sum_c (x_ic - c_jc)^2 + eps,
 *   u_ij = (dmin_i / d_ij)^exponent / sum_j (dmin_i / d_ij)^exponent,
 *
 * which is 1 / sum_j (d_ij / d_il)^exponent without its overflow.  labels[i]
 * (N int64, may be NULL) is the first index of the smallest d_ij; U (N x K in
 * dtype, leading dimension ldu, may be NULL) receives u_ij; sums (K x D
 * float64) and counts (K float64) receive sum_i u_ij^weight_power x_i and
 * sum_i u_ij^weight_power -- overwritten when zero_first is set, else added to.
 * points is never written; bytes beyond column D of a row are not read.
 *
 * float32 points: distances (difference form), memberships and the weighted
 * sums within one row tile are float32; everything above a row tile -- the
 * per-group partials, the counts and their reduction -- is float64.  float64
 * points: float64 throughout.  No atomics and a fixed reduction order: a
 * call's result is bitwise reproducible.  No load is wider than an element,
 * so any base address and leading dimension are served by the same kernel.
 *
 * spx_fuzzy_plan (pure host): the rows of a row tile, the number of row groups
 * (one persistent workgroup each), kmax (256) and the workspace bytes, which
 * depend on dtype, D, K and groups only.  kmax, row_tile and groups are
 * answered even where the call returns an error for K.
 *
 * Arguments are checked before any device work: SPX_EINVAL for a dtype code
 * out of range, N < 0, D < 1, K < 1, an exponent, eps or weight_power that is
 * not finite and > 0, ldp < D, ldu < K (with U), a null sums / counts /
 * points / centers pointer, or a short or misaligned workspace; SPX_ENOTSUP
 * for a dtype other than float32 / float64, K > kmax or D > 1048576.  N == 0
 * reads no points pointer, launches nothing and clears sums / counts when
 * zero_first is set.  Additive since ABI 3. */
int spx_fuzzy_plan(int dtype, int64_t N, int64_t D, int64_t K, int64_t* row_tile, int64_t* groups, int64_t* kmax,
                   size_t* workspace_bytes);
int spx_fuzzy_step(int dtype, int64_t N, int64_t D, int64_t K, const void* points, int64_t ldp, const double* centers,
                   double exponent, double eps, double weight_power, int64_t* labels, void* U, int64_t ldu,
                   double* sums, double* counts, int zero_first, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ------------------------------------------- n-body direct summation
 * Replaces the expression graph of the reference's n-body driver
 * (spartan/examples/nbody.py move()), a dozen (n, n) arrays per time step, by
 * one all-pairs kernel that reads 4 n values and writes 3 n.
 *
 * spx_nbody_accel: tx, ty, tz (n_tgt) are the targets' coordinates, sx, sy,
 * sz, sm (n_src) the sources' coordinates and masses, all contiguous vectors
 * of dtype (float32 / float64); the targets may be the sources.  For target j
 *
 *   d_i = s_i - t_j,  r_i = |d_i|,  r_i = rmin where r_i < rmin,
 *   a_j = sum_i G sm_i d_i / r_i^3
 *
 * is stored to ax, ay, az (n_tgt, dtype).  A pair at distance 0 contributes
 * exactly 0 when rmin > 0 (d = 0, r = rmin), so a target that is one of the
 * sources needs no index test; with rmin == 0 such a pair is 0 / 0 = NaN.
 * r < rmin is false for NaN: a NaN coordinate or mass makes every output NaN.
 * r^3 is never formed ((G m) / r / r / r * d), so float32 data with G m near
 * 1e20 and r near 1e14 stays in range; r^2 itself must not overflow dtype.
 *
 * A workgroup owns tgt_per_block targets and one of `splits` contiguous source
 * ranges.  splits == 0 takes spx_nbody_plan's choice (enough workgroups for
 * the CUs, no range shorter than 128 sources); a positive value forces it.
 * With splits > 1 the float64 partials [split][3][n_tgt] go to the workspace
 * and a second kernel adds them in ascending split order.  Sums of more than
 * 32 terms are carried in float64 in both dtypes.  No atomics: the same
 * inputs and split give bitwise identical outputs.
 *
 * spx_nbody_plan (pure host): *splits is read (NULL or 0: choose; positive:
 * forced) and receives the value used; workspace_bytes the bytes spx_nbody_accel
 * needs for it (0 for one split).
 *
 * Checked before any device work: SPX_EINVAL for a dtype code out of range, a
 * negative size, splits outside 0 .. 1024, a G that is not finite, an rmin
 * that is not finite and >= 0, a null pointer among the arrays that are read
 * or written, or a short or misaligned workspace; SPX_ENOTSUP for a dtype
 * other than float32 / float64, n_tgt above 2^31 - 1 workgroups' worth or
 * n_src above 2^48.  n_tgt == 0 launches nothing; n_src == 0 writes zeros.
 * Additive since ABI 3. */
int spx_nbody_plan(int dtype, int64_t n_tgt, int64_t n_src, int64_t* tgt_per_block, int64_t* splits,
                   size_t* workspace_bytes);
int spx_nbody_accel(int dtype, int64_t n_tgt, const void* tx, const void* ty, const void* tz, int64_t n_src,
                    const void* sx, const void* sy, const void* sz, const void* sm, double G, double rmin, void* ax,
                    void* ay, void* az, int64_t splits, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------ pairwise kernels
 * The two fixed computations behind the `shuffle` calls of the reference's
 * spectral clustering (spartan/examples/spectral_clustering.py: the Python
 * double loop of _row_similarity_mapper and the scaling of _laplacian_mapper),
 * and a cdist / pairwise_kernels primitive of its own.
 *
 * spx_pairwise: X is (n, d) with leading dimension ldx, Y is (m, d) with
 * leading dimension ldy, both row-major of dtype (float32 / float64); Y may be
 * X.  With s_ij = sum_k (x_ik - y_jk)^2 the value a_ij is */
#define SPX_PAIR_SQEUCLIDEAN 0 /* s_ij                      */
#define SPX_PAIR_EUCLIDEAN 1   /* sqrt(s_ij)                */
#define SPX_PAIR_MANHATTAN 2   /* sum_k |x_ik - y_jk|       */
#define SPX_PAIR_RBF 3         /* exp(-gamma s_ij)          */
/* evaluated in the difference form, k = 0 .. d - 1 in one order for every
 * element: equal rows give exactly 0 (rbf: exactly 1), and with Y == X the
 * result is bitwise symmetric.  gamma is read by rbf only.
 *
 *   row_scale (n), col_scale (m): both NULL or both given; the value becomes
 *     a_ij * (row_scale_i * col_scale_j), the product of the scales first;
 *   out (n, m; leading dimension ldo; may be NULL) receives the values;
 *     with diag_col0 >= 0 element (i, diag_col0 + i) receives diag_value
 *     instead (a row slab that starts at global row diag_col0);
 *   row_sums (n; may be NULL) receives sum_j of the values -- the computed
 *     ones, not diag_value.
 *
 * A workgroup owns `tile` rows and one of `splits` column ranges of whole
 * tiles, which it walks in ascending order, d staged k_chunk values at a time.
 * Sums above one tile are carried in float64.  splits == 0 takes
 * spx_pairwise_plan's choice (enough workgroups for the CUs, no range shorter
 * than four tiles); a positive value forces it.  With row_sums and splits > 1
 * the float64 partials [split][n] go to the workspace and a second kernel adds
 * them in ascending split order.  No atomics: the same inputs and split give
 * bitwise identical outputs.  A NaN coordinate makes that point's row (in X)
 * or column (in Y) NaN and nothing else of out; rbf of an overflowing
 * gamma * s is 0.
 *
 * spx_pairwise_plan (pure host): tile and k_chunk receive the kernel's tile
 * edge and k-chunk; *splits is read (NULL or 0: choose; positive: forced) and
 * receives the value used; workspace_bytes the bytes a call with row_sums needs
 * for it (0 for one split; a call without row_sums needs none).
 *
 * Checked before any device work: SPX_EINVAL for a dtype code out of range, a
 * negative size, splits outside 0 .. 1024, an unknown metric, d < 1, a gamma
 * that is not finite and >= 0, out and row_sums both NULL, one scale without
 * the other, ldx or ldy below d, ldo below m, a null X or Y, or a short or
 * misaligned workspace; SPX_ENOTSUP for a dtype other than float32 / float64,
 * n above 2^31 - 1 workgroups' worth or m above 2^48.  n == 0 or m == 0
 * succeeds and launches nothing.  Additive since ABI 3. */
int spx_pairwise_plan(int dtype, int64_t n, int64_t m, int64_t* tile, int64_t* k_chunk, int64_t* splits,
                      size_t* workspace_bytes);
int spx_pairwise(int dtype, int metric, int64_t n, int64_t m, int64_t d, const void* X, int64_t ldx, const void* Y,
                 int64_t ldy, double gamma, void* out, int64_t ldo, void* row_sums, const void* row_scale,
                 const void* col_scale, int64_t diag_col0, double diag_value, int64_t splits, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ------------------------------------------------------ automatic tiling */
/* Host-only (no device work, callable without a GPU): the node choice on the
 * AutomaticTiling cost graph (spartan/expr/optimize.py:454-890), replacing
 * the reference's native `tiling.mincost_tiling` (spartan/expr/tiling.cc:
 * 94-132, choice procedure :31-92).  Nodes 0..t, 0 = source, t = sink;
 * edge i is eu[i] -> ev[i] with cost ecost[i] (elements moved), in insertion
 * order; split pair k = {su[k], sv[k]} (the row / column alternatives of one
 * expression).  On return chosen[u] (u < t) is 1 for the chosen nodes and
 * *total_cost (may be NULL) holds the cost.  -1 on a malformed graph. */
int spx_mincost_tiling(int32_t t, int64_t n_edges, const int32_t* eu, const int32_t* ev, const int64_t* ecost,
                       int64_t n_split, const int32_t* su, const int32_t* sv, uint8_t* chosen,
                       int64_t* total_cost);

/* ----------------------------------------------------------- collectives
 * RCCL over xGMI, one communicator per process (one process per GPU).  The
 * reference has no collectives: every exchange below replaces a pattern of
 * pickled ZeroMQ point-to-point messages merged at an owner tile --
 *   partials of an axis reduction sent to the output tiles' owners and merged
 *     with np.add / np.minimum / np.maximum (reduce.py:53-67 ->
 *     distarray.py:384-421 -> tile.pyx:201-298): spx_reduce_scatter (row-slab
 *     outputs), spx_allreduce (others);
 *   dot partials reduced to the target tile's owner (map.py:326-328 with
 *     target reducer np.add, dot.py:268-283): spx_reduce / spx_reduce_scatter;
 *   argmin / argmax (value, index) partials gathered for the device combine
 *     (builtins.py:610-666): spx_allgather;
 *   a replicated small operand (the NumPy array2 pickled into every
 *     RunKernelReq, dot.py:249-257; k-means centres, k_means_.py:150-151):
 *     spx_broadcast;
 *   DistArray.fetch / update of remote regions (distarray.py:290-421 over
 *     blob_ctx.get / update): spx_sendrecv (one grouped point-to-point batch).
 * RCCL is opened at run time: spx_comm_load(path) dlopens it (NULL path:
 * "librccl.so.1"); the compute entry points never need it.  Counts are in
 * elements of dtype; ops are SPX_OP_SUM / MIN / MAX; all calls are enqueued
 * on `stream` (in-place send == recv allowed as in RCCL). */
int spx_comm_load(const char* rccl_path);
int spx_comm_unique_id(uint8_t* out, int64_t nbytes);          /* nbytes >= 128 */
int spx_comm_init(const uint8_t* unique_id, int64_t nbytes, int rank, int world, void** comm_out);
int spx_comm_destroy(void* comm);
int spx_allreduce(void* comm, const void* send, void* recv, int64_t count, int dtype, int op, void* stream);
int spx_reduce_scatter(void* comm, const void* send, void* recv, int64_t recvcount, int dtype, int op,
                       void* stream);
int spx_allgather(void* comm, const void* send, void* recv, int64_t sendcount, int dtype, void* stream);
int spx_broadcast(void* comm, const void* send, void* recv, int64_t count, int dtype, int root, void* stream);
int spx_reduce(void* comm, const void* send, void* recv, int64_t count, int dtype, int op, int root, void* stream);
/* grouped point-to-point: nsend byte buffers to speers[i], nrecv from rpeers[i] */
int spx_sendrecv(void* comm, int nsend, const void* const* sbufs, const int64_t* sbytes, const int* speers,
                 int nrecv, void* const* rbufs, const int64_t* rbytes, const int* rpeers, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPX_H */

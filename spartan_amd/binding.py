"""The binding of libspx.so (C ABI, include/spx.h): everything that talks to
the library and needs no GPU.

The ctypes signature table and ``load_library``, the dtype codes and
conversions, the error / pointer / stream helpers every caller of the ABI
shares (``backend.HipBackend``, ``comm``), and the host-only queries: the
tiling solver and the plans, limits and workspace sizes the library answers
without a device.  It imports nothing else of the package, and fails loudly
if the library is missing -- there is no CPU fallback.  (Not named ``libspx``:
``import spartan_amd.libspx`` would find libspx.so beside it first, as an
extension module.)
"""
import ctypes
import os
import threading

import numpy as np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libspx.so')

SPX_BOOL, SPX_I32, SPX_I64, SPX_F32, SPX_F64 = 0, 1, 2, 3, 4
OP_CODE = {'sum': 0, 'min': 1, 'max': 2, 'argmin': 3, 'argmax': 4, 'replace': 5}
FILL_CONST, FILL_ARANGE, FILL_UNIFORM, FILL_NORMAL = 0, 1, 2, 3

_DT = {np.dtype(np.bool_): SPX_BOOL, np.dtype(np.int32): SPX_I32, np.dtype(np.int64): SPX_I64,
       np.dtype(np.float32): SPX_F32, np.dtype(np.float64): SPX_F64}
_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def spx_dtype(dt):
  dt = np.dtype(dt)
  if dt not in _DT:
    raise TypeError('dtype %s is not supported by the MI355X backend '
                    '(bool, int32, int64, float32, float64)' % dt)
  return _DT[dt]


_TORCH_DT, _NP_DT = {}, {}  # NumPy dtype <-> torch dtype, filled on first use (torch is imported lazily)


def _dtype_tables():
  import torch
  # (int8 / uint8 / int16: generated kernels only -- codegen.CTYPE lowers them, spx_dtype does not take them)
  pairs = [(np.dtype(name), getattr(torch, name))
           for name in ('bool', 'int32', 'int64', 'float32', 'float64', 'int8', 'uint8', 'int16')]
  _NP_DT.update((t, d) for d, t in pairs)
  _TORCH_DT.update(pairs)


def torch_dtype(dt):
  _TORCH_DT or _dtype_tables()
  return _TORCH_DT[np.dtype(dt)]


def np_dtype(tdt):
  _NP_DT or _dtype_tables()
  return _NP_DT[tdt]


# ------------------------------------------------------------------ library
_lib = None
_lib_lock = threading.Lock()

_I64P = ctypes.POINTER(ctypes.c_int64)


def _signatures():
  """{name: (argument types, result type)} in the order of include/spx.h
  (tests/test_abi.py checks every entry against the header's prototype)."""
  I, I32, U32, I64, U64, SZ, F64 = (ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64,
                                    ctypes.c_size_t, ctypes.c_double)
  VP, CP = ctypes.c_void_p, ctypes.c_char_p
  VPP, IP, I32P, U8P, F64P = (ctypes.POINTER(t) for t in (VP, I, I32, ctypes.c_uint8, F64))
  return {
      'spx_abi_version': ([], I),
      'spx_last_error': ([], CP),
      'spx_module_load': ([VP, SZ, VPP], I),
      'spx_module_unload': ([VP], I),
      'spx_module_function': ([VP, CP, VPP], I),
      'spx_launch': ([VP, U32, U32, U32, U32, U32, VP, SZ, VP], I),
      'spx_fill': ([I, I, VP, I, _I64P, _I64P, _I64P, F64, F64, U64, VP], I),
      'spx_reduce_finalize': ([I, I, I, VP, VP, I64, I64, VP, VP, VP], I),
      'spx_reduce_finalize_pair': ([I, VP, I64, I64, VP, VP, I64, I64, VP, VP], I),
      'spx_merge': ([I, I, VP, VP, I, _I64P, _I64P, _I64P, VP, I, I, VP], I),
      'spx_copy_region': ([I, VP, _I64P, _I64P, I, VP, _I64P, _I64P, I, _I64P, VP], I),
      'spx_gemm': ([I, I64, I64, I64, VP, I64, VP, I64, VP, I64, F64, F64, VP], I),
      'spx_gemm_plan': ([I, I64, I64, I64, VP, I64, VP, I64] + [_I64P] * 6, I),
      'spx_argreduce_combine': ([I, I, VP, VP, I64, I64, VP, VP, VP], I),
      'spx_kmeans_assign_workspace': ([I, I64, I64, I64], I64),
      'spx_kmeans_assign': ([I, I64, I64, I64, VP, I64, VP, VP, VP, VP, SZ, I, VP], I),
      'spx_kmeans_accumulate_workspace': ([I, I64, I64, I64], I64),
      'spx_kmeans_accumulate': ([I, I64, I64, I64, VP, I64, VP, VP, VP, I, VP, SZ, VP], I),
      'spx_kmeans_step_workspace': ([I, I64, I64, I64], I64),
      'spx_kmeans_step': ([I, I64, I64, I64, VP, I64, VP, VP, VP, VP, I, VP, SZ, I, VP], I),
      'spx_kmeans_timing': ([I], I),
      'spx_kmeans_times': ([F64P, F64P, I], I),
      'spx_cdist': ([I, I, I64, I64, I64, VP, I64, VP, VP, I64, VP], I),
      'spx_bincount': ([VP, I64, I64, VP, I, VP], I),
      'spx_scan_workspace': ([I, I64, I64, I64], I64),
      'spx_scan': ([I, VP, VP, I64, I64, I64, VP, VP, I, VP, SZ, VP], I),
      'spx_sort_workspace': ([I, I64, I64, I64, I], I64),
      'spx_sort': ([I, VP, VP, VP, I64, I64, I64, VP, SZ, VP], I),
      'spx_sort_plan': ([I, I64, I64, I64, _I64P, _I64P], I),
      'spx_topk_workspace': ([I, I64, I64, I64, I64, I], I64),
      'spx_topk': ([I, VP, VP, VP, VP, I64, I64, I64, I64, I, VP, SZ, VP], I),
      'spx_topk_plan': ([I, I64, I64, I64, I64, _I64P, _I64P], I),
      'spx_knn_workspace': ([I, I64, I64, I64, I64], I64),
      'spx_knn': ([I, I64, I64, I64, I64, VP, I64, VP, I64, VP, VP, VP, SZ, VP], I),
      'spx_knn_plan': ([I, I64, I64, I64, I64, _I64P, _I64P], I),
      'spx_take': ([I, I, VP, VP, VP, I64, I64, I64, I64, I64, I64, I64, I64, VP, VP], I),
      'spx_compact_workspace': ([I64], I64),
      'spx_compact_count': ([VP, I64, VP, VP, SZ, VP], I),
      'spx_compact': ([I, VP, VP, VP, I64, I64, I64, I64, VP, SZ, VP], I),
      'spx_stencil_plan': ([I, _I64P, _I64P, _I64P], I),
      'spx_stencil': ([I, VP, VP, VP, I64, I64, I64, I64, I64, I64, I64, VP], I),
      'spx_maxpool': ([I, VP, VP, I64, I64, I64, I64, I64, VP], I),
      'spx_potrf_plan': ([I, _I64P, _I64P], I),
      'spx_potrf_workspace': ([I, I64], I64),
      'spx_potrf': ([I, I64, VP, I64, VP, I64, VP, VP, SZ, VP], I),
      'spx_trsm_workspace': ([I, I, I64, I64], I64),
      'spx_trsm': ([I, I, I, I64, I64, VP, I64, VP, I64, VP, SZ, VP], I),
      'spx_syrk': ([I, I, I64, I64, I64, VP, I64, VP, I64, VP, I64, VP], I),
      'spx_geqr_plan': ([I, I64, _I64P, _I64P], I),
      'spx_geqr_workspace': ([I, I64, I64], I64),
      'spx_geqr': ([I, I64, I64, VP, I64, VP, I64, VP, SZ, VP], I),
      'spx_orgqr': ([I, I64, I64, VP, SZ, VP, I64, VP, I64, VP], I),
      'spx_syevj_plan': ([I, _I64P, _I64P], I),
      'spx_syevj': ([I, I, I64, I64, VP, I64, I64, VP, I64, VP, I64, I64, VP, VP], I),
      'spx_gesvj_plan': ([I, I64, _I64P, _I64P, _I64P], I),
      'spx_gesvj': ([I, I, I64, I64, I64, VP, I64, I64, VP, I64, I64, VP, I64, VP, I64, I64, VP, VP], I),
      'spx_csrmm_plan': ([I, I64, I64, I64, _I64P, _I64P, _I64P], I),
      'spx_csrmm_workspace': ([I, I64, I64, I64], I64),
      'spx_csrmm': ([I, I64, I64, I64, I64, VP, VP, VP, VP, I64, VP, I64, F64, F64, I64, VP, SZ, I, VP], I),
      'spx_csr_todense': ([I, I64, I64, I64, VP, VP, VP, VP, I64, VP], I),
      'spx_csr_rowids': ([I64, I64, VP, I64, VP, VP], I),
      'spx_als_plan': ([I, I64, _I64P, _I64P], I),
      'spx_als_solve': ([I, I64, I64, I64, I64, VP, VP, VP, VP, I64, F64, VP, I64, VP, VP], I),
      'spx_apsp_plan': ([I, _I64P], I),
      'spx_apsp': ([I, I, I64, VP, I64, VP, I64, F64, VP, VP], I),
      'spx_fuzzy_plan': ([I, I64, I64, I64, _I64P, _I64P, _I64P, ctypes.POINTER(SZ)], I),
      'spx_fuzzy_step': ([I, I64, I64, I64, VP, I64, VP, F64, F64, F64, VP, VP, I64, VP, VP, I, VP, SZ, VP], I),
      'spx_nbody_plan': ([I, I64, I64, _I64P, _I64P, ctypes.POINTER(SZ)], I),
      'spx_nbody_accel': ([I, I64, VP, VP, VP, I64, VP, VP, VP, VP, F64, F64, VP, VP, VP, I64, VP, SZ, VP], I),
      'spx_pairwise_plan': ([I, I64, I64, _I64P, _I64P, _I64P, ctypes.POINTER(SZ)], I),
      'spx_pairwise': ([I, I, I64, I64, I64, VP, I64, VP, I64, F64, VP, I64, VP, VP, VP, I64, F64, I64, VP, SZ, VP], I),
      'spx_comm_load': ([CP], I),
      'spx_comm_unique_id': ([VP, I64], I),
      'spx_comm_init': ([VP, I64, I, I, VPP], I),
      'spx_comm_destroy': ([VP], I),
      'spx_allreduce': ([VP, VP, VP, I64, I, I, VP], I),
      'spx_reduce_scatter': ([VP, VP, VP, I64, I, I, VP], I),
      'spx_allgather': ([VP, VP, VP, I64, I, VP], I),
      'spx_broadcast': ([VP, VP, VP, I64, I, I, VP], I),
      'spx_reduce': ([VP, VP, VP, I64, I, I, I, VP], I),
      'spx_sendrecv': ([VP, I, VPP, _I64P, IP, I, VPP, _I64P, IP, VP], I),
      'spx_mincost_tiling': ([I32, I64, I32P, I32P, _I64P, I64, I32P, I32P, U8P, _I64P], I),
  }


_SIGS = _signatures()
EXPORTED = tuple(_SIGS)


def load_library(path=LIB_PATH):
  """Load libspx.so (importing torch first so its HIP runtime is the one used)."""
  global _lib
  with _lib_lock:
    if _lib is not None:
      return _lib
    import torch  # noqa: F401  (torch's libamdhip64.so.7 must be the loaded runtime)
    if not os.path.exists(path):
      raise RuntimeError('libspx.so not found at %s: run __graft_entry__.build() '
                         '(hipcc --offload-arch=gfx950); there is no CPU fallback' % path)
    lib = ctypes.CDLL(path)
    for name, (args, res) in _SIGS.items():
      fn = getattr(lib, name)
      fn.argtypes = args
      fn.restype = res
    _lib = lib
    return lib


# ------------------------------------------------- error / argument helpers
def _check(rc, what):
  if rc != 0:
    raise RuntimeError('%s failed (%d): %s' % (what, rc, _lib.spx_last_error().decode()))


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _arr(vals):
  vals = [int(v) for v in vals] or [0]
  return (ctypes.c_int64 * len(vals))(*vals)


def current_stream():
  # the raw pointer of the current stream, without building a torch Stream
  # object (torch.cuda.current_stream() cost ~10 us per call, three calls
  # per lreg iteration)
  import torch
  return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


# ------------------------------------------------------------ tiling solver
def mincost_tiling(t, edges, split_pairs):
  """spx_mincost_tiling (host code in libspx.so, no GPU needed): the node
  choice of the AutomaticTiling cost graph.  edges: [(u, v, cost)] in
  insertion order; split_pairs: [(a, b)].  Returns (chosen node ids < t,
  total cost)."""
  lib = load_library()
  n = len(edges)
  I32 = ctypes.c_int32
  eu = (I32 * max(n, 1))(*[int(e[0]) for e in edges])
  ev = (I32 * max(n, 1))(*[int(e[1]) for e in edges])
  ec = (ctypes.c_int64 * max(n, 1))(*[int(e[2]) for e in edges])
  m = len(split_pairs)
  su = (I32 * max(m, 1))(*[int(p[0]) for p in split_pairs])
  sv = (I32 * max(m, 1))(*[int(p[1]) for p in split_pairs])
  chosen = (ctypes.c_uint8 * max(int(t), 1))()
  total = ctypes.c_int64(0)
  rc = lib.spx_mincost_tiling(int(t), n, eu, ev, ec, m, su, sv, chosen, ctypes.byref(total))
  if rc != 0:
    raise ValueError('spx_mincost_tiling: malformed tiling graph')
  return [u for u in range(int(t)) if chosen[u]], int(total.value)


# ------------------------------------------- plans, limits, workspace sizes
SCAN_CHUNK = 32768  # elements of a line per chunk of a chunked scan (csrc/scan_kernels.h)


def scan_dtypes(dt):
  """(result dtype, accumulator dtype) of a cumulative sum over ``dt``:
  np.cumsum's result dtype; carries and totals are int64 / float64."""
  dt = np.dtype(dt)
  spx_dtype(dt)
  if dt.kind == 'f':
    return dt, np.dtype(np.float64)
  return np.dtype(np.int64), np.dtype(np.int64)


def scan_plan(outer, n, inner, dtype):
  """(mode, chunk) spx_scan uses for an (outer, n, inner) scan of ``dtype``:
  'line' (one pass, a workgroup or wave walks whole lines; chunk == n) or
  'chunked' (lines cut into SCAN_CHUNK elements over three launches).  The
  library decides from the geometry and the CU count; a chunked scan is the
  one that needs a workspace."""
  need = load_library().spx_scan_workspace(spx_dtype(dtype), int(outer), int(n), int(inner))
  if need < 0:
    raise ValueError('scan_plan: bad geometry (%s, %s, %s)' % (outer, n, inner))
  return ('chunked', SCAN_CHUNK) if need > 0 else ('line', int(n))


SORT_LDS_MAX = 2048  # longest line spx_sort sorts in LDS (csrc/sort_kernels.h)
SORT_TILE = 16384    # keys per workgroup and radix pass (csrc/sort_kernels.h)


def sort_plan(outer, n, inner, dtype, want_idx=False):
  """(path, passes) spx_sort uses for an (outer, n, inner) sort of ``dtype``:
  ('lds', 0) -- lines of at most SORT_LDS_MAX keys, sorted in LDS, no
  workspace -- or ('radix', passes), least-significant-digit passes over
  tiles of SORT_TILE keys.  The library's own answer (spx_sort_plan);
  ``want_idx`` changes the workspace, not the path."""
  rc = load_library().spx_sort_plan(spx_dtype(dtype), int(outer), int(n), int(inner), None, None)
  if rc < 0:
    raise ValueError('sort_plan: bad geometry (%s, %s, %s)' % (outer, n, inner))
  return ('radix', rc) if rc > 0 else ('lds', 0)


def topk_plan(outer, n, inner, dtype, k=1):
  """(path, passes, chunk) spx_topk uses for an (outer, n, inner) selection
  of ``dtype``: ('lds', 0, chunk) -- lines of at most SORT_LDS_MAX elements,
  sorted in LDS -- or ('select', passes, chunk), most-significant-digit radix
  select passes over chunks of ``chunk`` elements (spx_topk_plan)."""
  chunk = ctypes.c_int64(0)
  rc = load_library().spx_topk_plan(spx_dtype(dtype), int(outer), int(n), int(inner), int(k), None,
                                    ctypes.byref(chunk))
  if rc < 0:
    raise ValueError('topk_plan: bad geometry (%s, %s, %s), k %s' % (outer, n, inner, k))
  return ('select', rc, int(chunk.value)) if rc > 0 else ('lds', 0, int(chunk.value))


def knn_plan(Q, N, D, k, dtype=np.float32):
  """(number of point ranges, range length) of spx_knn (spx_knn_plan)."""
  chunk = ctypes.c_int64(0)
  rc = load_library().spx_knn_plan(spx_dtype(dtype), int(Q), int(N), int(D), int(k), None, ctypes.byref(chunk))
  if rc < 0:
    raise ValueError('knn_plan: bad arguments (Q %s, N %s, D %s, k %s)' % (Q, N, D, k))
  return rc, int(chunk.value)


def _k_limit(which):
  """TOPK_K_MAX / KNN_K_MAX: the library's own limits, through the plan calls."""
  if which in globals():
    return globals()[which]
  kmax = ctypes.c_int64(0)
  lib = load_library()
  if which == 'TOPK_K_MAX':
    lib.spx_topk_plan(SPX_F32, 1, 1, 1, 1, ctypes.byref(kmax), None)
  else:
    lib.spx_knn_plan(SPX_F32, 1, 1, 1, 1, ctypes.byref(kmax), None)
  globals()[which] = int(kmax.value)
  return int(kmax.value)


def compact_tile():
  """Mask bytes per workgroup of spx_compact_count / spx_compact
  (COMPACT_TILE in csrc/index_kernels.h), read from the library: the
  workspace starts with one int64 per tile, so the tile is the longest mask
  whose workspace is a single entry.  Also ``backend.COMPACT_TILE``."""
  ws = load_library().spx_compact_workspace
  lo, hi = 1, 1 << 40  # ws(lo) == 8 < ws(hi)
  while hi - lo > 1:
    mid = (lo + hi) // 2
    if ws(mid) <= 8:
      lo = mid
    else:
      hi = mid
  return lo


GEMM_KERNELS = ('NONE', 'INT', 'F32_SMALL', 'F32_BIG', 'F32_P3', 'F64', 'F64_P3')  # SPX_GEMM_* of include/spx.h


def gemm_plan(dtype, M, N, K, a_ptr=256, lda=None, b_ptr=256, ldb=None):
  """The route spx_gemm takes for an (M, K) @ (K, N) product of ``dtype``
  (spx_gemm_plan, the library's own selection): a dict of 'kernel' (a name of
  GEMM_KERNELS), 'aligned' (the instantiation without bounds checks), the
  block tile 'bm', 'bn', 'bk' and 'flush_k' (the K distance between the
  kernel's flushes into C; 0: one chain over any K).  ``a_ptr`` / ``b_ptr``
  are addresses (``tensor.data_ptr()``) of which only the alignment counts,
  ``lda`` / ``ldb`` the row strides in elements (default: contiguous)."""
  lda, ldb = (K if lda is None else lda), (N if ldb is None else ldb)
  v = [ctypes.c_int64(0) for _ in range(6)]
  rc = load_library().spx_gemm_plan(spx_dtype(dtype), int(M), int(N), int(K), ctypes.c_void_p(int(a_ptr)), int(lda),
                                    ctypes.c_void_p(int(b_ptr)), int(ldb), *[ctypes.byref(x) for x in v])
  if rc != 0:
    raise ValueError('gemm_plan (%d): %s' % (rc, _lib.spx_last_error().decode()))
  kernel, aligned, bm, bn, bk, flush_k = (int(x.value) for x in v)
  return {'kernel': GEMM_KERNELS[kernel], 'aligned': bool(aligned), 'bm': bm, 'bn': bn, 'bk': bk, 'flush_k': flush_k}


def _float_plan(op, kernel, dtype, nout, sizes=(), negative=None):
  """The ``nout`` int64 answers of spx_<op>_plan, which has kernels for
  float32 / float64 only (``kernel``: what the TypeError calls them), for the
  integer ``sizes`` (``negative``: the ValueError's wording when one is < 0)."""
  dt = np.dtype(dtype)
  if dt not in _FLOATS:
    raise TypeError('%s_plan: dtype %s has no %s kernel (float32 / float64)' % (op, dt, kernel))
  sizes = tuple(int(s) for s in sizes)
  if sizes and min(sizes) < 0:
    raise ValueError('%s_plan: %s' % (op, negative % sizes))
  v = [ctypes.c_int64(0) for _ in range(nout)]
  name = 'spx_%s_plan' % op
  _check(getattr(load_library(), name)(spx_dtype(dt), *sizes, *[ctypes.byref(x) for x in v]), name)
  return tuple(int(x.value) for x in v)


def stencil_plan(dtype):
  """(bm, bn, bk): the block tile of spx_stencil for ``dtype`` (float32 /
  float64) -- rows of F, columns of W * H and the K-tile of C * fw * fh
  (StencilTile in csrc/stencil_kernels.h), read from the library."""
  return _float_plan('stencil', 'stencil', dtype, 3)


def potrf_plan(dtype):
  """(nb, nb_outer): the diagonal block one workgroup factors in LDS and the
  outer panel (the K of the trailing update) of spx_potrf, from the library."""
  return _float_plan('potrf', 'Cholesky', dtype, 2)


def geqr_plan(dtype, n):
  """(nmax, r) of spx_geqr for ``n`` columns of ``dtype``, from the library:
  the column limit and the rows one workgroup factors in LDS (r >= 2 n; 0 where
  n is above the limit)."""
  return _float_plan('geqr', 'QR', dtype, 2, (n,), 'negative n = %d')


def syevj_plan(dtype):
  """(nmax, sweep_max) of spx_syevj for ``dtype``, from the library: the
  largest n one workgroup holds in LDS and the bound on the sweeps."""
  return _float_plan('syevj', 'eigen-solver', dtype, 2)


def gesvj_plan(dtype, n):
  """(nmax, mmax, sweep_max) of spx_gesvj for ``n`` columns of ``dtype``, from
  the library: the column limit, the most rows one workgroup holds in LDS beside
  the n x n V (0 where n is above the limit) and the bound on the sweeps."""
  return _float_plan('gesvj', 'SVD', dtype, 3, (n,), 'negative n = %d')


def csrmm_plan(dtype, m, nnz, p):
  """(g, T, rows_per_block) of spx_csrmm for an (m, .) CSR matrix of ``nnz``
  nonzeros times ``p`` dense columns, from the library: the lanes that work on
  one row, the row length above which a row is cut into chunks of T for whole
  workgroups, and the rows one workgroup covers."""
  return _float_plan('csrmm', 'sparse', dtype, 3, (m, nnz, p), 'negative size (%d, %d, %d)')


def als_plan(dtype, f):
  """(fmax, rows_per_block) of spx_als_solve for ``f`` features of ``dtype``,
  from the library: the largest f the kernel holds in a wave's registers and
  the rows one workgroup solves (0 where f is outside 1 .. fmax)."""
  return _float_plan('als', 'ALS', dtype, 2, (f,), 'negative f = %d')


def apsp_plan(dtype):
  """The pivot-block edge b of spx_apsp for ``dtype``, from the library: the
  matrix is processed in ceil(n / b) rounds of b x b tiles."""
  return _float_plan('apsp', 'shortest-path', dtype, 1)[0]


def fuzzy_plan(dtype, N, D, K):
  """(row_tile, groups, kmax, workspace bytes) of spx_fuzzy_step for (N, D)
  points of ``dtype`` and K centres, from the library: the rows over which the
  float32 accumulators of a group live, the number of row groups (persistent
  workgroups), the largest K and the workspace, which depends on dtype, D, K
  and groups only.  For K above kmax the first three are still answered and
  the workspace is None."""
  dt = np.dtype(dtype)
  if dt not in _FLOATS:
    raise TypeError('fuzzy_plan: dtype %s has no fuzzy k-means kernel (float32 / float64)' % dt)
  N, D, K = int(N), int(D), int(K)
  if N < 0 or D < 1 or K < 1:
    raise ValueError('fuzzy_plan: bad sizes (N %d, D %d, K %d)' % (N, D, K))
  rt, g, kmax = (ctypes.c_int64(0) for _ in range(3))
  nbytes = ctypes.c_size_t(0)
  rc = load_library().spx_fuzzy_plan(spx_dtype(dt), N, D, K, ctypes.byref(rt), ctypes.byref(g), ctypes.byref(kmax),
                                     ctypes.byref(nbytes))
  if rc != 0 and K <= kmax.value:
    _check(rc, 'spx_fuzzy_plan')
  return int(rt.value), int(g.value), int(kmax.value), (int(nbytes.value) if rc == 0 else None)


def nbody_plan(dtype, n_tgt, n_src, splits=0):
  """(tgt_per_block, splits, workspace bytes) of spx_nbody_accel for ``n_tgt``
  targets against ``n_src`` sources of ``dtype``, from the library: the targets
  one workgroup owns, the contiguous source ranges the work is cut into
  (``splits`` 0: the library's choice; positive: forced) and the bytes of the
  float64 partials (0 for one range)."""
  dt = np.dtype(dtype)
  if dt not in _FLOATS:
    raise TypeError('nbody_plan: dtype %s has no n-body kernel (float32 / float64)' % dt)
  n_tgt, n_src, splits = int(n_tgt), int(n_src), int(splits)
  if n_tgt < 0 or n_src < 0:
    raise ValueError('nbody_plan: negative size (n_tgt %d, n_src %d)' % (n_tgt, n_src))
  tpb, s = ctypes.c_int64(0), ctypes.c_int64(splits)
  nbytes = ctypes.c_size_t(0)
  _check(load_library().spx_nbody_plan(spx_dtype(dt), n_tgt, n_src, ctypes.byref(tpb), ctypes.byref(s),
                                       ctypes.byref(nbytes)), 'spx_nbody_plan')
  return int(tpb.value), int(s.value), int(nbytes.value)


PAIR_METRICS = {'sqeuclidean': 0, 'euclidean': 1, 'manhattan': 2, 'rbf': 3}  # SPX_PAIR_* of include/spx.h


def pairwise_plan(dtype, n, m, splits=0):
  """(tile, k_chunk, splits, workspace bytes) of spx_pairwise for (n, d)
  against (m, d) points of ``dtype``, from the library: the edge of the square
  tile of pairs a workgroup computes at a time (it owns ``tile`` rows), the
  values of k staged at a time, the contiguous column ranges the work is cut
  into (``splits`` 0: the library's choice; positive: forced) and the bytes of
  the float64 row-sum partials a call with ``row_sums`` needs (0 for one
  range)."""
  dt = np.dtype(dtype)
  if dt not in _FLOATS:
    raise TypeError('pairwise_plan: dtype %s has no pairwise kernel (float32 / float64)' % dt)
  n, m, splits = int(n), int(m), int(splits)
  if n < 0 or m < 0:
    raise ValueError('pairwise_plan: negative size (n %d, m %d)' % (n, m))
  tile, kc, s = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(splits)
  nbytes = ctypes.c_size_t(0)
  _check(load_library().spx_pairwise_plan(spx_dtype(dt), n, m, ctypes.byref(tile), ctypes.byref(kc), ctypes.byref(s),
                                          ctypes.byref(nbytes)), 'spx_pairwise_plan')
  return int(tile.value), int(kc.value), int(s.value), int(nbytes.value)


def __getattr__(name):
  if name == 'COMPACT_TILE':
    globals()['COMPACT_TILE'] = t = compact_tile()
    return t
  if name in ('TOPK_K_MAX', 'KNN_K_MAX'):
    return _k_limit(name)
  raise AttributeError('module %r has no attribute %r' % (__name__, name))

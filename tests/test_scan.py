"""``spartan_amd.scan`` host logic (no GPU): the reference's KAT
(tests/test_scan.py there), the tile-wise restatement of spartan/expr/scan.py
over several tile layouts and dtypes, laziness and validation, the plan cache,
two gloo ranks, and the C-ABI argument checks of spx_scan.

The expression layer runs here over the CPU test double with a NumPy ``scan``
(scan_ref.ScanFakeBackend); the kernels themselves are tested on the GPU in
tests/test_scan_gpu.py.
"""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, 'spartan_amd', 'libspx.so')

AXES = (None, 0, 1)


@pytest.fixture
def scan_ctx(host_ctx):
  """host_ctx with the scan-capable test double installed."""
  from spartan_amd import backend
  from scan_ref import ScanFakeBackend

  def make(num_workers=1):
    ctx = host_ctx(num_workers)
    backend.set_backend(ScanFakeBackend())
    return ctx
  return make


# ------------------------------------------------------------ reference KAT
@pytest.mark.parametrize('W', [1, 2, 3, 4])
def test_reference_kat(scan_ctx, W):
  scan_ctx(W)
  import spartan_amd
  from spartan_amd import expr
  a = np.ones((10, 10), np.float32)
  for axis in AXES:
    x = expr.from_numpy(a, tile_hint=(5, 5))
    got = spartan_amd.scan(x, np.sum, np.cumsum, axis=axis).glom()
    want = np.cumsum(a, axis=axis).reshape(a.shape)
    assert got.dtype == np.float32 and got.shape == a.shape
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------- tile-wise restatement
def _values(shape, dtype, seed):
  r = np.random.RandomState(seed)
  n = int(np.prod(shape))
  if dtype == np.bool_:
    return (r.randint(0, 2, n) > 0).reshape(shape)
  if dtype == np.float64:
    # multiples of 1/8 below 2^20: every partial sum is exact in fp64, so
    # the result does not depend on the order of the additions
    return (r.randint(-2 ** 23, 2 ** 23, n) / 8.0).reshape(shape)
  if dtype == np.int32:
    return r.randint(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32).reshape(shape)
  return r.randint(-2 ** 40, 2 ** 40, n, dtype=np.int64).reshape(shape)


CASES = [
    ((40, 30), [None, (7, 30), (40, 8), (9, 11), (1, 30), (40, 1)]),
    ((7,), [None, (2,), (7,), (1,)]),
    ((3, 10, 12), [None, (3, 4, 12), (1, 10, 5), (2, 3, 7), (3, 10, 1)]),
]


@pytest.mark.parametrize('dtype', [np.int64, np.int32, np.bool_, np.float64])
@pytest.mark.parametrize('W', [1, 3])
def test_matches_tilewise_restatement(scan_ctx, dtype, W):
  scan_ctx(W)
  from spartan_amd import expr
  from scan_ref import flat_cumsum, scan_tiles
  for shape, hints in CASES:
    a = _values(shape, dtype, 7 + len(shape))
    for hint in hints:
      for axis in (None,) + tuple(range(len(shape))) + (-1,):
        x = expr.from_numpy(a, tile_hint=hint)
        e = expr.scan(x, axis=axis)
        got = e.glom()
        want = scan_tiles(a, axis, hint, W)
        direct = flat_cumsum(a) if axis is None else np.cumsum(a, axis=axis)
        assert got.dtype == want.dtype == direct.dtype == e.dtype, (got.dtype, want.dtype, direct.dtype)
        np.testing.assert_array_equal(got, want, err_msg='%s %s %s' % (shape, hint, axis))
        np.testing.assert_array_equal(got, direct, err_msg='%s %s %s' % (shape, hint, axis))


@pytest.mark.parametrize('W', [1, 3])
def test_int64_above_2p53(scan_ctx, W):
  """500 values of 2^53 + 1: the sum stays below 2^63 and any float path
  would drop the ones."""
  scan_ctx(W)
  from spartan_amd import expr
  a = np.full((500,), 2 ** 53 + 1, np.int64)
  for hint in (None, (37,), (250,)):
    got = expr.scan(expr.from_numpy(a, tile_hint=hint), axis=0).glom()
    np.testing.assert_array_equal(got, (2 ** 53 + 1) * np.arange(1, 501, dtype=np.int64))
    got = expr.scan(expr.from_numpy(a.reshape(20, 25), tile_hint=None if hint is None else (3, 7))).glom()
    np.testing.assert_array_equal(got.reshape(-1), (2 ** 53 + 1) * np.arange(1, 501, dtype=np.int64))


# ------------------------------------------------- laziness and validation
def test_lazy_shape_dtype_and_composition(scan_ctx):
  scan_ctx(2)
  from spartan_amd import backend, expr
  from spartan_amd.expr.scan import ScanExpr
  a = np.arange(1200, dtype=np.int32).reshape(40, 30) % 17
  x = expr.from_numpy(a, tile_hint=(9, 30))
  be = backend.get()
  n0 = len(be.calls)
  e = expr.scan(x)
  assert isinstance(e, ScanExpr) and isinstance(e, expr.Expr)
  assert e.shape == (40, 30) and e.dtype == np.int64
  f = expr.scan(x * 2, axis=0)
  assert f.shape == (40, 30) and f.dtype == np.cumsum(a * 2, axis=0).dtype
  g = expr.scan(expr.from_numpy(a.astype(np.float32)), axis=-1)
  assert g.dtype == np.float32 and g.axis == 1
  assert len(be.calls) == n0 and e.cache() is None and f.cache() is None  # nothing ran
  got = (f + 1).sum().glom()
  assert got == (np.cumsum(a * 2, axis=0) + 1).sum()
  assert 'scan' in be.calls[n0:]
  # a view as the input is evaluated through the normal path first
  v = expr.scan(x[3:29, 4:20].T, axis=1).glom()
  np.testing.assert_array_equal(v, np.cumsum(a[3:29, 4:20].T, axis=1))
  # a host array is accepted like everywhere else in the API; a map over one
  # is a replicated array (one tile held by every rank)
  np.testing.assert_array_equal(expr.scan(a, axis=1).glom(), np.cumsum(a, axis=1))
  for axis in AXES:
    got = expr.scan(expr.as_array(a) * 2, axis=axis).glom()
    np.testing.assert_array_equal(got, np.cumsum(a * 2, axis=axis).reshape(a.shape))


def test_axis_out_of_range(scan_ctx):
  scan_ctx(1)
  from spartan_amd import expr
  x = expr.from_numpy(np.ones((4, 5)))
  for bad in (5, 2, -3):
    with pytest.raises(ValueError):
      expr.scan(x, axis=bad)
  assert expr.scan(x, axis=-2).axis == 0


@pytest.mark.parametrize('W', [1, 3])
def test_other_callables_take_the_host_path(scan_ctx, W):
  scan_ctx(W)
  from spartan_amd import backend, expr
  from scan_ref import scan_tiles
  red = lambda t, axis=None: np.sum(t, axis=axis)  # noqa: E731
  scn = lambda t, axis=None: np.cumsum(t, axis=axis)  # noqa: E731
  a = _values((40, 30), np.int64, 3)
  be = backend.get()
  for hint in (None, (9, 11)):
    for axis in AXES:
      n0 = len(be.calls)
      got = expr.scan(expr.from_numpy(a, tile_hint=hint), red, scn, axis=axis).glom()
      assert 'scan' not in be.calls[n0:]  # not the device path
      np.testing.assert_array_equal(got, scan_tiles(a, axis, hint, W, red, scn))
      np.testing.assert_array_equal(got, np.cumsum(a, axis=axis).reshape(a.shape))


# ---------------------------------------------------------------- plan cache
def test_plan_cache_hit(scan_ctx):
  scan_ctx(3)
  from spartan_amd import expr
  from spartan_amd.expr import plan_cache
  a = _values((40, 30), np.int64, 5)
  X = expr.lazify(expr.from_numpy(a, tile_hint=(9, 30)).force())
  plan_cache.clear()
  h0, m0 = plan_cache.STATS['hits'], plan_cache.STATS['misses']
  r1 = (expr.scan(X * 2, axis=0) + 1).optimized().glom()
  assert plan_cache.STATS['misses'] == m0 + 1
  r2 = (expr.scan(X * 2, axis=0) + 1).optimized().glom()
  assert plan_cache.STATS['hits'] == h0 + 1
  np.testing.assert_array_equal(r1, r2)
  np.testing.assert_array_equal(r1, np.cumsum(a * 2, axis=0) + 1)
  # another axis is another structure
  r3 = (expr.scan(X * 2, axis=1) + 1).optimized().glom()
  assert plan_cache.STATS['misses'] == m0 + 2
  np.testing.assert_array_equal(r3, np.cumsum(a * 2, axis=1) + 1)


# --------------------------------------------------------------- gloo ranks
def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _gloo_body(rank, world, port, W, q):
  try:
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank), SPARTAN_SPMD_GUARD='strict',
                      SPARTAN_NCCL_TIMEOUT='240')
    from spartan_amd import backend, runtime, expr
    from spartan_amd.config import FLAGS
    from scan_ref import ScanFakeBackend, scan_tiles
    backend.set_backend(ScanFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    ctx = runtime.get()
    assert ctx.world_size == world and ctx.dist_backend == 'gloo'
    for dtype in (np.int64, np.float64):
      a = _values((40, 30), dtype, 11)
      for hint in (None, (7, 30), (40, 8), (9, 11)):
        for axis in AXES:
          x = expr.from_numpy(a, tile_hint=hint).force()
          got = expr.scan(x, axis=axis).glom()
          np.testing.assert_array_equal(got, scan_tiles(a, axis, hint, W), err_msg='%s %s' % (hint, axis))
          np.testing.assert_array_equal(got, np.cumsum(a, axis=axis).reshape(a.shape))
      # a lazy input and a host-path pair over ranks
      x = expr.from_numpy(a, tile_hint=(9, 11))
      np.testing.assert_array_equal(expr.scan(x + x, axis=0).glom(), np.cumsum(a + a, axis=0))
      got = expr.scan(x, lambda t, axis=None: np.sum(t, axis=axis), lambda t, axis=None: np.cumsum(t, axis=axis),
                      axis=1).glom()
      np.testing.assert_array_equal(got, np.cumsum(a, axis=1))
    q.put((rank, 'ok'))
  except Exception:  # pragma: no cover - reported to the parent
    import traceback
    q.put((rank, traceback.format_exc()))
  finally:
    try:
      from spartan_amd import runtime
      runtime.shutdown()
    except Exception:
      pass


@pytest.mark.parametrize('W', [2, 3])
def test_world2_gloo_scan(W):
  import multiprocessing as mp
  ctx = mp.get_context('spawn')
  q = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_gloo_body, args=(r, 2, port, W, q)) for r in range(2)]
  for p in procs:
    p.start()
  res = {}
  for _ in procs:
    r, msg = q.get(timeout=240)
    res[r] = msg
  for p in procs:
    p.join(timeout=60)
  for r in range(2):
    assert res.get(r) == 'ok', res.get(r)


# ------------------------------------------------------------ ABI, no GPU
def _scan_lib():
  import torch  # noqa: F401  (torch's HIP runtime first)
  lib = ctypes.CDLL(LIB)
  lib.spx_last_error.restype = ctypes.c_char_p
  lib.spx_scan_workspace.restype = ctypes.c_int64
  lib.spx_scan_workspace.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
  lib.spx_scan.restype = ctypes.c_int
  lib.spx_scan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                           ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                           ctypes.c_size_t, ctypes.c_void_p]
  return lib


@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_scan_argument_validation_without_gpu():
  """Bad arguments are rejected before any device work (code + message).
  The pointers are host buffers: a call that got past its checks would try to
  launch on them, so every case here must stop at a check."""
  lib = _scan_lib()
  buf = (ctypes.c_double * 16)()
  p = ctypes.cast(buf, ctypes.c_void_p)
  rc = lib.spx_scan(99, p, p, 1, 4, 1, None, None, 0, None, 0, None)
  assert rc == -1 and b'dtype' in lib.spx_last_error()
  rc = lib.spx_scan(3, p, p, 1, 0, 1, None, None, 0, None, 0, None)
  assert rc == -1 and b'geometry' in lib.spx_last_error()
  assert lib.spx_scan(3, p, p, 0, 4, 1, None, None, 0, None, 0, None) == -1
  assert lib.spx_scan(3, p, p, 1, 4, -2, None, None, 0, None, 0, None) == -1
  rc = lib.spx_scan(3, p, None, 1, 4, 1, None, None, 0, None, 0, None)
  assert rc == -1 and b'both null' in lib.spx_last_error()
  rc = lib.spx_scan(3, None, p, 1, 4, 1, None, None, 0, None, 0, None)
  assert rc == -1 and b'null input' in lib.spx_last_error()
  # a chunked geometry without (or with too small a) workspace
  from spartan_amd import backend
  n = 4 * backend.SCAN_CHUNK
  need = lib.spx_scan_workspace(3, 1, n, 1)
  assert need > 0
  rc = lib.spx_scan(3, p, p, 1, n, 1, None, None, 0, None, 0, None)
  assert rc == -1 and b'workspace' in lib.spx_last_error()
  rc = lib.spx_scan(3, p, p, 1, n, 1, None, None, 0, p, need - 1, None)
  assert rc == -1 and b'workspace' in lib.spx_last_error()
  assert lib.spx_scan_workspace(3, 1, 1000, 1) >= 0
  assert lib.spx_scan_workspace(4, 5, 64, 257) >= 0
  assert lib.spx_scan_workspace(3, 1, 0, 1) < 0
  assert lib.spx_scan_workspace(99, 1, 8, 1) < 0
  assert lib.spx_scan_workspace(3, 2 ** 40, 2 ** 40, 2 ** 40) < 0


@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_scan_plan_and_chunk_constant():
  """backend.scan_plan reports the library's own choice, and
  backend.SCAN_CHUNK is the library's chunk length: one line of C elements is
  a single pass, C + 1 elements are two chunks of 8-byte totals."""
  from spartan_amd import backend
  C = backend.SCAN_CHUNK
  lib = _scan_lib()
  assert lib.spx_scan_workspace(3, 1, C, 1) == 0
  assert lib.spx_scan_workspace(3, 1, C + 1, 1) == 16
  assert lib.spx_scan_workspace(0, 2, 3 * C + 17, 3) == 2 * 4 * 3 * 8
  assert backend.scan_plan(1, C, 1, np.float32) == ('line', C)
  assert backend.scan_plan(1, C + 1, 1, np.float32) == ('chunked', C)
  assert backend.scan_plan(5, 3 * C + 17, 3, np.int64) == ('chunked', C)
  assert backend.scan_plan(5, 257, 64, np.float64) == ('line', 257)
  assert backend.scan_plan(100000, C + 1, 1, np.float32) == ('line', C + 1)  # enough lines: one pass
  with pytest.raises(ValueError):
    backend.scan_plan(1, 0, 1, np.float32)
  assert backend.scan_dtypes(np.bool_) == (np.dtype(np.int64), np.dtype(np.int64))
  assert backend.scan_dtypes(np.float32) == (np.dtype(np.float32), np.dtype(np.float64))
  assert 'spx_scan' in backend.EXPORTED and 'spx_scan_workspace' in backend.EXPORTED

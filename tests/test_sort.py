"""``spartan_amd.sort`` / ``argsort`` / ``partition`` / ``argpartition`` host
logic (no GPU): the reference's KAT (tests/test_sort.py there) over tile
layouts the reference cannot sort, axis=None, the partition contract,
laziness and validation, the plan cache, two gloo ranks, and the C-ABI
argument checks of spx_sort / spx_sort_workspace / spx_sort_plan.

The expression layer runs here over the CPU test double with a NumPy ``sort``
(sort_ref.SortFakeBackend); the kernels themselves are tested on the GPU in
tests/test_sort_gpu.py.
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


@pytest.fixture
def sort_ctx(host_ctx):
  """host_ctx with the sort-capable test double installed."""
  from spartan_amd import backend
  from sort_ref import SortFakeBackend

  def make(num_workers=1):
    ctx = host_ctx(num_workers)
    backend.set_backend(SortFakeBackend())
    return ctx
  return make


def _kat_shapes():
  """2-d to 5-d shapes with sides 5..10, fixed seed (the reference draws
  them with randint(5, 10) per dimension)."""
  r = np.random.RandomState(1234)
  return [tuple(int(s) for s in r.randint(5, 11, nd)) for nd in range(2, 6)]


def _hints(shape):
  """Tile layouts of one shape: default, whole-line tiles for the last and
  the first axis, cuts along one axis, a block layout (two axes cut), and
  (1, n) / (n, 1) style tiles."""
  nd = len(shape)
  hints = [None,
           tuple(2 if d == 0 else s for d, s in enumerate(shape)),        # whole lines along every axis but 0
           tuple(3 if d == nd - 1 else s for d, s in enumerate(shape)),   # cut along the last axis only
           tuple(3 if d < 2 else s for d, s in enumerate(shape)),         # blocks: cut along axes 0 and 1
           tuple(1 if d == 0 else s for d, s in enumerate(shape)),        # (1, n, ...)
           tuple(1 if d == nd - 1 else s for d, s in enumerate(shape))]   # (..., n, 1)
  return hints


# ------------------------------------------------------------ reference KAT
@pytest.mark.parametrize('W', [1, 3])
def test_reference_kat_every_axis_and_layout(sort_ctx, W):
  sort_ctx(W)
  from spartan_amd import expr
  from sort_ref import kat_ints
  for si, shape in enumerate(_kat_shapes()):
    a = kat_ints(shape, 7 + si)
    for hint in _hints(shape):
      for axis in tuple(range(len(shape))) + (-1,):
        x = expr.from_numpy(a, tile_hint=hint)
        s = expr.sort(x, axis)
        got = s.glom()
        assert got.dtype == a.dtype == s.dtype and got.shape == a.shape == s.shape
        np.testing.assert_array_equal(got, np.sort(a, axis), err_msg='%s %s %s' % (shape, hint, axis))
        g = expr.argsort(x, axis)
        idx = g.glom()
        assert idx.dtype == np.int64 == g.dtype and idx.shape == a.shape
        np.testing.assert_array_equal(idx, np.argsort(a, axis, kind='stable'),
                                      err_msg='%s %s %s' % (shape, hint, axis))


@pytest.mark.parametrize('W', [1, 3])
def test_one_dimensional_array_in_several_tiles(sort_ctx, W):
  """The reference sorts such an array tile by tile; NumPy's result is the
  contract here.  Heavy duplicates: the argsort must be the stable one."""
  sort_ctx(W)
  from spartan_amd import expr
  r = np.random.RandomState(3)
  a = r.randint(-5, 6, 1000).astype(np.int64)
  for hint in (None, (1000,), (37,), (250,), (1,)):
    x = expr.from_numpy(a, tile_hint=hint)
    for axis in (0, -1):
      np.testing.assert_array_equal(expr.sort(x, axis).glom(), np.sort(a))
      np.testing.assert_array_equal(expr.argsort(x, axis).glom(), np.argsort(a, kind='stable'))
    np.testing.assert_array_equal(expr.sort(x).glom(), np.sort(a))  # the default axis is the last one


@pytest.mark.parametrize('W', [1, 3])
def test_result_keeps_the_input_layout(sort_ctx, W):
  sort_ctx(W)
  from spartan_amd import expr
  from sort_ref import kat_ints
  a = kat_ints((40, 30), 5)
  for hint in ((7, 30), (40, 8), (9, 11)):
    x = expr.from_numpy(a, tile_hint=hint).force()
    for axis in (0, 1):
      for fn in (expr.sort, expr.argsort):
        res = fn(expr.lazify(x), axis).force()
        assert res.tiles == x.tiles, (hint, axis)


@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.int32, np.bool_])
def test_dtypes_nans_and_zeros(sort_ctx, dtype):
  sort_ctx(3)
  from spartan_amd import expr
  from sort_ref import neg_zero_count, sort_data
  a = sort_data((1, 40, 30), dtype, 'extremes', 11).reshape(40, 30)
  for hint in (None, (9, 11)):
    for axis in (0, 1):
      x = expr.from_numpy(a, tile_hint=hint)
      got = expr.sort(x, axis).glom()
      assert got.dtype == a.dtype
      np.testing.assert_array_equal(got, np.sort(a, axis))
      idx = expr.argsort(x, axis).glom()
      np.testing.assert_array_equal(idx, np.argsort(a, axis, kind='stable'))
      if np.dtype(dtype).kind == 'f':
        np.testing.assert_array_equal(neg_zero_count(got, axis), neg_zero_count(a, axis))


# ------------------------------------------------------------ axis = None
@pytest.mark.parametrize('W', [1, 3])
def test_axis_none_is_the_flat_sort(sort_ctx, W):
  sort_ctx(W)
  from spartan_amd import expr
  from sort_ref import kat_ints
  for shape, hint in (((40, 30), (9, 11)), ((7,), (2,)), ((3, 10, 12), (2, 3, 7)), ((40, 30), None)):
    a = kat_ints(shape, 2)
    e = expr.sort(expr.from_numpy(a, tile_hint=hint), axis=None)
    assert e.shape == (a.size,) and e.dtype == a.dtype
    got = e.glom()
    assert got.shape == (a.size,)
    np.testing.assert_array_equal(got, np.sort(a, axis=None))
  x = expr.from_numpy(kat_ints((4, 5), 1))
  with pytest.raises(AssertionError, match="doesn't support argsort when axis == None"):
    expr.argsort(x, axis=None)


# ------------------------------------------------- partition / argpartition
@pytest.mark.parametrize('W', [1, 3])
def test_partition_contract(sort_ctx, W):
  sort_ctx(W)
  from spartan_amd import expr
  from sort_ref import kat_ints
  a = kat_ints((20, 17, 6), 9)
  x = expr.from_numpy(a, tile_hint=(6, 5, 6))
  for axis in (0, 1, 2, -1):
    n = a.shape[axis]
    for kth in (0, n // 2, n - 1, -1):
      k = kth % n
      want = np.take(np.sort(a, axis), [k], axis)  # each line's kth smallest, kept as an axis of length 1
      idx = expr.argpartition(x, kth, axis).glom()
      assert idx.dtype == np.int64
      for p in (expr.partition(x, kth, axis).glom(), np.take_along_axis(a, idx, axis)):
        assert p.shape == a.shape and p.dtype == a.dtype
        np.testing.assert_array_equal(np.sort(p, axis), np.sort(a, axis))  # a permutation of each line
        np.testing.assert_array_equal(np.take(p, [k], axis), want)         # the kth element in its sorted place
        before = np.take(p, np.arange(0, k), axis)
        after = np.take(p, np.arange(k + 1, n), axis)
        assert (before <= want).all() and (after >= want).all()
  for bad in (17, -18, 1.5):
    with pytest.raises(ValueError):
      expr.partition(x, bad, axis=1)
    with pytest.raises(ValueError):
      expr.argpartition(x, bad, axis=1)
  assert expr.partition(x, (0, 16), axis=1).shape == a.shape
  for fn in (expr.partition, expr.argpartition):
    with pytest.raises(AssertionError, match='axis == None'):
      fn(x, 1, axis=None)


# ------------------------------------------------- laziness and validation
def test_lazy_shape_dtype_and_composition(sort_ctx):
  sort_ctx(2)
  import spartan_amd
  from spartan_amd import backend, expr
  from spartan_amd.expr.sort import SortExpr
  assert spartan_amd.sort is expr.sort and spartan_amd.argsort is expr.argsort
  a = (np.arange(1200, dtype=np.int32).reshape(40, 30) * 7919) % 173
  x = expr.from_numpy(a, tile_hint=(9, 11))
  be = backend.get()
  n0 = len(be.calls)
  e = expr.sort(x, axis=0)
  f = expr.argsort(x * 2)
  assert isinstance(e, SortExpr) and isinstance(e, expr.Expr)
  assert e.shape == (40, 30) and e.dtype == np.int32 and e.axis == 0
  assert f.shape == (40, 30) and f.dtype == np.int64 and f.axis == 1
  assert len(be.calls) == n0 and e.cache() is None and f.cache() is None  # nothing ran
  got = (expr.sort(x * 2, axis=0) + 1).glom()
  np.testing.assert_array_equal(got, np.sort(a * 2, axis=0) + 1)
  assert 'sort' in be.calls[n0:]
  np.testing.assert_array_equal(f.glom(), np.argsort(a * 2, axis=1, kind='stable'))
  # a view as the input is evaluated through the normal path first
  v = a[3:29, 4:20].T
  np.testing.assert_array_equal(expr.sort(x[3:29, 4:20].T, axis=1).glom(), np.sort(v, axis=1))
  np.testing.assert_array_equal(expr.argsort(x[3:29, 4:20].T, axis=0).glom(), np.argsort(v, axis=0, kind='stable'))
  np.testing.assert_array_equal((expr.sort(x * 2, axis=0) + 1).optimized().glom(), np.sort(a * 2, axis=0) + 1)
  # a host array, and a map over one (a replicated array: one tile held by every rank)
  np.testing.assert_array_equal(expr.sort(a, axis=1).glom(), np.sort(a, axis=1))
  for axis in (None, 0, 1):
    np.testing.assert_array_equal(expr.sort(expr.as_array(a) * 2, axis=axis).glom(), np.sort(a * 2, axis=axis))
  np.testing.assert_array_equal(expr.argsort(expr.as_array(a) * 2, axis=0).glom(),
                                np.argsort(a * 2, axis=0, kind='stable'))


def test_validation_errors(sort_ctx):
  sort_ctx(1)
  from spartan_amd import expr
  x = expr.from_numpy(np.ones((4, 5)))
  for fn in (expr.sort, expr.argsort):
    for bad in (5, 2, -3, 1.0, 'x'):
      with pytest.raises(ValueError):
        fn(x, axis=bad)
    assert fn(x, axis=-2).axis == 0
    with pytest.raises(ValueError):
      fn(np.float64(3.0))  # 0-d
  with pytest.raises(ValueError):
    expr.sort(np.float64(3.0), axis=None)
  with pytest.raises(TypeError):
    expr.sort(expr.from_numpy(np.ones((4, 5))).force().glom().astype(np.complex128)).glom()


# ---------------------------------------------------------------- plan cache
def test_plan_cache_keys_axis_and_kind(sort_ctx):
  sort_ctx(3)
  from spartan_amd import expr
  from spartan_amd.expr import plan_cache
  from sort_ref import kat_ints
  a = kat_ints((40, 30), 5)
  X = expr.lazify(expr.from_numpy(a, tile_hint=(9, 30)).force())
  plan_cache.clear()
  h0, m0 = plan_cache.STATS['hits'], plan_cache.STATS['misses']
  r1 = (expr.sort(X * 2, axis=0) + 1).optimized().glom()
  assert plan_cache.STATS['misses'] == m0 + 1
  r2 = (expr.sort(X * 2, axis=0) + 1).optimized().glom()
  assert plan_cache.STATS['hits'] == h0 + 1
  np.testing.assert_array_equal(r1, r2)
  np.testing.assert_array_equal(r1, np.sort(a * 2, axis=0) + 1)
  # another axis is another structure
  r3 = (expr.sort(X * 2, axis=1) + 1).optimized().glom()
  assert plan_cache.STATS['misses'] == m0 + 2
  np.testing.assert_array_equal(r3, np.sort(a * 2, axis=1) + 1)
  # and argsort is not sort
  r4 = (expr.argsort(X * 2, axis=0) + 1).optimized().glom()
  assert plan_cache.STATS['misses'] == m0 + 3 and plan_cache.STATS['hits'] == h0 + 1
  np.testing.assert_array_equal(r4, np.argsort(a * 2, axis=0, kind='stable') + 1)
  r5 = (expr.argsort(X * 2, axis=0) + 1).optimized().glom()
  assert plan_cache.STATS['hits'] == h0 + 2
  np.testing.assert_array_equal(r4, r5)


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
    from sort_ref import SortFakeBackend, kat_ints
    backend.set_backend(SortFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    ctx = runtime.get()
    assert ctx.world_size == world and ctx.dist_backend == 'gloo'
    a = kat_ints((40, 30), 11)
    for hint in (None, (7, 30), (40, 8), (9, 11)):
      for axis in (0, 1, None):
        x = expr.from_numpy(a, tile_hint=hint).force()
        np.testing.assert_array_equal(expr.sort(x, axis).glom(), np.sort(a, axis), err_msg='%s %s' % (hint, axis))
        if axis is not None:
          np.testing.assert_array_equal(expr.argsort(x, axis).glom(), np.argsort(a, axis, kind='stable'))
    b = kat_ints((1000,), 12) % 9
    for hint in (None, (37,)):
      x = expr.from_numpy(b, tile_hint=hint)
      np.testing.assert_array_equal(expr.sort(x).glom(), np.sort(b))
      np.testing.assert_array_equal(expr.argsort(x).glom(), np.argsort(b, kind='stable'))
    x = expr.from_numpy(a, tile_hint=(9, 11))
    np.testing.assert_array_equal((expr.sort(x + x, axis=0) + 1).glom(), np.sort(a + a, axis=0) + 1)
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
def test_world2_gloo_sort(W):
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
def _sort_lib():
  import torch  # noqa: F401  (torch's HIP runtime first)
  lib = ctypes.CDLL(LIB)
  lib.spx_last_error.restype = ctypes.c_char_p
  lib.spx_sort_workspace.restype = ctypes.c_int64
  lib.spx_sort_workspace.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
  lib.spx_sort.restype = ctypes.c_int
  lib.spx_sort.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                           ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
  lib.spx_sort_plan.restype = ctypes.c_int
  lib.spx_sort_plan.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
  return lib


@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_sort_argument_validation_without_gpu():
  """Bad arguments are rejected before any device work (code + message).
  The pointers are host buffers: a call that got past its checks would try to
  launch on them, so every case here must stop at a check."""
  from spartan_amd import backend
  lib = _sort_lib()
  bufs = [(ctypes.c_double * 16)() for _ in range(3)]
  p, v, i = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
  EINVAL, ENOTSUP = -1, -3
  rc = lib.spx_sort(99, p, v, i, 1, 4, 1, None, 0, None)
  assert rc == EINVAL and b'dtype' in lib.spx_last_error()
  for geom in ((-1, 4, 1), (1, -4, 1), (1, 4, -2), (2 ** 40, 2 ** 30, 2 ** 40)):
    rc = lib.spx_sort(3, p, v, i, *geom, None, 0, None)
    assert rc == EINVAL and b'geometry' in lib.spx_last_error(), geom
  rc = lib.spx_sort(3, None, v, i, 1, 4, 1, None, 0, None)
  assert rc == EINVAL and b'null input' in lib.spx_last_error()
  rc = lib.spx_sort(3, p, None, None, 1, 4, 1, None, 0, None)
  assert rc == EINVAL and b'both null' in lib.spx_last_error()
  rc = lib.spx_sort(3, p, p, None, 1, 4, 1, None, 0, None)
  assert rc == EINVAL and b'alias' in lib.spx_last_error()
  rc = lib.spx_sort(2, p, None, p, 1, 4, 1, None, 0, None)
  assert rc == EINVAL and b'alias' in lib.spx_last_error()
  rc = lib.spx_sort(3, p, v, i, 1, 2 ** 31, 1, None, 0, None)
  assert rc == ENOTSUP and b'2^31' in lib.spx_last_error()
  # a radix geometry without (or with too small a) workspace
  n = backend.SORT_LDS_MAX + 1
  for want_idx, oi in ((0, None), (1, i)):
    need = lib.spx_sort_workspace(3, 1, n, 1, want_idx)
    assert need > 0
    rc = lib.spx_sort(3, p, v, oi, 1, n, 1, None, 0, None)
    assert rc == EINVAL and b'workspace' in lib.spx_last_error()
    rc = lib.spx_sort(3, p, v, oi, 1, n, 1, p, need - 1, None)
    assert rc == EINVAL and b'workspace' in lib.spx_last_error()
  # nothing to sort: SPX_OK without a launch, whatever the pointers are
  for geom in ((1, 0, 1), (0, 4, 1), (1, 4, 0), (3, 0, 5)):
    assert lib.spx_sort(3, p, v, i, *geom, None, 0, None) == 0, geom
    assert lib.spx_sort_workspace(3, *geom, 1) == 0
  assert lib.spx_sort_workspace(99, 1, 8, 1, 0) < 0
  assert lib.spx_sort_workspace(3, -1, 8, 1, 0) < 0
  assert lib.spx_sort_workspace(3, 1, 2 ** 31, 1, 0) < 0
  assert lib.spx_sort_workspace(3, 2 ** 40, 2 ** 30, 2 ** 40, 0) < 0


@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_sort_plan_and_constants():
  """backend.sort_plan reports the library's own choice; SORT_LDS_MAX and
  SORT_TILE are the library's; the workspace holds what the passes need."""
  from spartan_amd import backend
  lib = _sort_lib()
  L, T = backend.SORT_LDS_MAX, backend.SORT_TILE
  lds, tile = ctypes.c_int64(0), ctypes.c_int64(0)
  assert lib.spx_sort_plan(3, 1, 8, 1, ctypes.byref(lds), ctypes.byref(tile)) == 0
  assert (lds.value, tile.value) == (L, T)
  for dt in (np.bool_, np.int32, np.int64, np.float32, np.float64):
    for inner in (1, 3):
      assert backend.sort_plan(5, 1, inner, dt) == ('lds', 0)
      assert backend.sort_plan(5, L, inner, dt, True) == ('lds', 0)
      assert lib.spx_sort_workspace(backend.spx_dtype(dt), 5, L, inner, 1) == 0
  passes = {np.bool_: 1, np.int32: 4, np.float32: 4, np.int64: 8, np.float64: 8}
  for dt, want in passes.items():
    assert backend.sort_plan(2, L + 1, 3, dt) == ('radix', want)
    assert backend.sort_plan(1, 3 * T + 5, 1, dt, True) == ('radix', want)
  with pytest.raises(ValueError):
    backend.sort_plan(1, -1, 1, np.float32)
  with pytest.raises(ValueError):
    backend.sort_plan(1, 2 ** 31, 1, np.float32)
  # two key buffers (+ two position buffers with indices) and the digit counts
  lines, n = 6, 2 * T + 9
  N = lines * n
  keys = lib.spx_sort_workspace(3, 2, n, 3, 0)
  both = lib.spx_sort_workspace(3, 2, n, 3, 1)
  counts = lines * 256 * 3 * 8
  assert 2 * 4 * N + counts <= keys <= 2 * 4 * N + counts + (1 << 20)
  assert 2 * 4 * N <= both - keys <= 2 * 4 * N + 512
  assert lib.spx_sort_workspace(4, 2, n, 3, 0) >= 2 * 8 * N + counts
  # one bool pass over contiguous lines goes from the input to the outputs: counts only;
  # strided lines are transposed into and out of the key buffers
  assert lib.spx_sort_workspace(0, 6, n, 1, 1) <= counts + (1 << 20)
  assert lib.spx_sort_workspace(0, 2, n, 3, 1) >= 2 * 4 * N + 2 * 4 * N + counts
  for name in ('spx_sort', 'spx_sort_workspace', 'spx_sort_plan'):
    assert name in backend.EXPORTED

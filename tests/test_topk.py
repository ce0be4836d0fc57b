"""``spartan_amd.topk`` / ``argtopk`` and ``NearestNeighbors`` host logic (no
GPU): the expression layer over tile layouts and worker counts, laziness and
validation, the ``k > TOPK_K_MAX`` fallback, two gloo ranks, and the C-ABI
argument checks of spx_topk / spx_knn and their workspace / plan calls.

The expression layer runs here over the CPU test double with NumPy ``topk`` /
``knn`` (topk_ref.TopkFakeBackend); the kernels themselves are tested on the
GPU in tests/test_topk_gpu.py.
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

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')


@pytest.fixture
def topk_ctx(host_ctx):
  """host_ctx with the topk-capable test double installed."""
  from spartan_amd import backend
  from topk_ref import TopkFakeBackend

  def make(num_workers=1):
    ctx = host_ctx(num_workers)
    backend.set_backend(TopkFakeBackend())
    return ctx
  return make


# ------------------------------------------------------------- expr layer
@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_topk_every_axis_and_layout(topk_ctx, W):
  topk_ctx(W)
  from spartan_amd import expr
  from sort_ref import kat_ints
  from topk_ref import topk_ref
  a = kat_ints((40, 30, 6), 3) % 17  # duplicates: the positions must be the stable ones
  hints = [None, (7, 30, 6), (40, 8, 6), (9, 11, 6), (40, 30, 1), (1, 30, 6)]  # cutting the axis and not
  for hint in hints:
    for axis in (0, 1, 2, -1):
      n = a.shape[axis]
      for k in (1, 3, n):
        for largest in (False, True):
          x = expr.from_numpy(a, tile_hint=hint)
          want_v, want_i = topk_ref(a, k, axis, largest)
          v = expr.topk(x, k, axis, largest)
          g = expr.argtopk(x, k, axis, largest)
          assert v.shape == want_v.shape == g.shape and v.dtype == a.dtype and g.dtype == np.int64
          got_v, got_i = v.glom(), g.glom()
          assert got_v.dtype == a.dtype and got_i.dtype == np.int64
          msg = '%s %s %s %s' % (hint, axis, k, largest)
          np.testing.assert_array_equal(got_v, want_v, err_msg=msg)
          np.testing.assert_array_equal(got_i, want_i, err_msg=msg)


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_one_dimensional_array_in_several_tiles(topk_ctx, W):
  topk_ctx(W)
  from spartan_amd import expr
  from topk_ref import topk_ref
  r = np.random.RandomState(3)
  a = r.randint(-5, 6, 1000).astype(np.int64)
  for hint in (None, (1000,), (37,), (250,)):
    x = expr.from_numpy(a, tile_hint=hint)
    for largest in (False, True):
      want_v, want_i = topk_ref(a, 20, 0, largest)
      np.testing.assert_array_equal(expr.topk(x, 20, 0, largest).glom(), want_v)
      np.testing.assert_array_equal(expr.argtopk(x, 20, largest=largest).glom(), want_i)


@needs_lib
@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.int32, np.bool_])
def test_dtypes_nans_zeros_and_int_min(topk_ctx, dtype):
  topk_ctx(3)
  from spartan_amd import expr
  from topk_ref import same_bits, sort_data, topk_ref
  a = sort_data((1, 40, 30), dtype, 'extremes', 11).reshape(40, 30)
  for hint in (None, (9, 11)):
    for axis in (0, 1):
      for largest in (False, True):
        x = expr.from_numpy(a, tile_hint=hint)
        want_v, want_i = topk_ref(a, 7, axis, largest)
        np.testing.assert_array_equal(expr.argtopk(x, 7, axis, largest).glom(), want_i)
        assert same_bits(expr.topk(x, 7, axis, largest).glom(), want_v)  # signs of zeros included


@needs_lib
def test_lazy_shape_dtype_replicated_and_composition(topk_ctx):
  topk_ctx(2)
  import spartan_amd
  from spartan_amd import backend, expr
  from spartan_amd.expr.topk import TopkExpr
  from topk_ref import topk_ref
  assert spartan_amd.topk is expr.topk and spartan_amd.argtopk is expr.argtopk
  a = (np.arange(1200, dtype=np.int32).reshape(40, 30) * 7919) % 173
  x = expr.from_numpy(a, tile_hint=(9, 11))
  be = backend.get()
  n0 = len(be.calls)
  e = expr.topk(x, 5, axis=0)
  f = expr.argtopk(x * 2, 4, largest=True)
  assert isinstance(e, TopkExpr) and isinstance(e, expr.Expr)
  assert e.shape == (5, 30) and e.dtype == np.int32 and e.axis == 0 and e.k == 5
  assert f.shape == (40, 4) and f.dtype == np.int64 and f.axis == 1 and f.largest
  assert len(be.calls) == n0 and e.cache() is None and f.cache() is None  # nothing ran
  got = (expr.topk(x * 2, 5, axis=0) + 1).glom()
  np.testing.assert_array_equal(got, topk_ref(a * 2, 5, 0)[0] + 1)
  assert 'topk' in be.calls[n0:] and 'sort' not in be.calls[n0:]
  np.testing.assert_array_equal(f.glom(), topk_ref(a * 2, 4, 1, True)[1])
  np.testing.assert_array_equal((expr.topk(x * 2, 5, axis=0) + 1).optimized().glom(), topk_ref(a * 2, 5, 0)[0] + 1)
  # a view, a host array, and a map over one (replicated: one tile held by every rank)
  v = a[3:29, 4:20].T
  np.testing.assert_array_equal(expr.argtopk(x[3:29, 4:20].T, 6, axis=0).glom(), topk_ref(v, 6, 0)[1])
  np.testing.assert_array_equal(expr.topk(a, 3, axis=1).glom(), topk_ref(a, 3, 1)[0])
  for axis in (0, 1):
    np.testing.assert_array_equal(expr.topk(expr.as_array(a) * 2, 3, axis=axis, largest=True).glom(),
                                  topk_ref(a * 2, 3, axis, True)[0])
    np.testing.assert_array_equal(expr.argtopk(expr.as_array(a) * 2, 3, axis=axis).glom(),
                                  topk_ref(a * 2, 3, axis)[1])


@needs_lib
def test_validation_errors(topk_ctx):
  topk_ctx(1)
  from spartan_amd import expr
  x = expr.from_numpy(np.ones((4, 5)))
  for fn in (expr.topk, expr.argtopk):
    for bad in (5, 2, -3, 1.0, 'x'):
      with pytest.raises(ValueError):
        fn(x, 1, axis=bad)
    for bad in (0, -1, 6, 1.5, True, None):
      with pytest.raises(ValueError):
        fn(x, bad, axis=1)
    with pytest.raises(ValueError):
      fn(x, 5, axis=0)  # k > n along that axis
    assert fn(x, 4, axis=-2).axis == 0
    with pytest.raises(ValueError):
      fn(np.float64(3.0), 1)  # 0-d
    with pytest.raises(AssertionError, match='axis == None'):
      fn(x, 1, axis=None)
  with pytest.raises(TypeError):
    expr.topk(np.ones((4, 5), np.complex128), 2).glom()


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_k_above_the_kernel_limit(topk_ctx, W):
  """largest=False goes through sort / argsort and a slice; largest=True is refused."""
  topk_ctx(W)
  from spartan_amd import backend, expr
  from topk_ref import topk_ref
  K = backend.TOPK_K_MAX
  assert K == backend.SORT_LDS_MAX
  r = np.random.RandomState(5)
  a = r.randint(-50, 50, (3, K + 40)).astype(np.int32)
  be = backend.get()
  for hint in (None, (3, 1000)):
    x = expr.from_numpy(a, tile_hint=hint)
    n0 = len(be.calls)
    want_v, want_i = topk_ref(a, K + 1, 1)
    v = expr.topk(x, K + 1, axis=1)
    assert v.shape == (3, K + 1) and v.dtype == np.int32
    np.testing.assert_array_equal(v.glom(), want_v)
    np.testing.assert_array_equal(expr.argtopk(x, K + 1).glom(), want_i)
    assert 'sort' in be.calls[n0:] and 'topk' not in be.calls[n0:]
    np.testing.assert_array_equal(expr.topk(x, K, axis=1).glom(), topk_ref(a, K, 1)[0])  # at the limit: selected
    assert 'topk' in be.calls[n0:]
    for fn in (expr.topk, expr.argtopk):
      with pytest.raises(NotImplementedError, match=str(K)):
        fn(x, K + 1, axis=1, largest=True)


# -------------------------------------------------------- NearestNeighbors
def _nn_check(X, q, k, hint, qhint=None, **kw):
  from spartan_amd import expr
  from spartan_amd.examples.neighbors import NearestNeighbors
  from topk_ref import knn_ref, same_bits
  s, want_i = knn_ref(X, q, k)
  nn = NearestNeighbors(**kw).fit(expr.from_numpy(X, tile_hint=hint))
  dist, ind = nn.kneighbors(expr.from_numpy(q, tile_hint=qhint), n_neighbors=k)
  assert dist.dtype == X.dtype and ind.dtype == np.int64 and dist.shape == ind.shape == (q.shape[0], k)
  np.testing.assert_array_equal(ind, want_i, err_msg='%s %s' % (hint, k))
  assert same_bits(dist, np.sqrt(s).astype(X.dtype))


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_nearest_neighbors_over_layouts(topk_ctx, W):
  topk_ctx(W)
  from spartan_amd import backend
  from topk_ref import knn_data
  for kind, dt in (('grid', np.float32), ('far', np.float32), ('nonfinite', np.float64), ('dup', np.float64)):
    X, q = knn_data(kind, 203, 9, 6, dt, 4)
    for hint in (None, (203, 6), (50, 6), (50, 4), (3, 6)):  # one tile, row tiles, row + column tiles, tiny blocks
      for k in (1, 5, 20):
        _nn_check(X, q, k, hint, qhint=(4, 6))
  be = backend.get()
  assert 'knn' in be.calls and 'sort' not in be.calls


@needs_lib
def test_nearest_neighbors_interface(topk_ctx):
  topk_ctx(2)
  from spartan_amd import backend, expr
  from spartan_amd.examples.neighbors import NearestNeighbors
  from topk_ref import knn_data, knn_ref
  X, q = knn_data('uniform', 120, 7, 5, np.float32, 8)
  want = knn_ref(X, q, 5)[1]
  outs = []
  for alg in ('auto', 'ball_tree', 'kd_tree', 'brute'):  # NumPy inputs, the constructor's default k
    nn = NearestNeighbors(algorithm=alg).fit(X)
    dist, ind = nn.kneighbors(q)
    assert ind.shape == (7, 5) and dist.dtype == np.float32
    np.testing.assert_array_equal(ind, want)
    outs.append(dist)
  for d in outs[1:]:
    np.testing.assert_array_equal(d, outs[0])
  nn = NearestNeighbors(n_neighbors=3).fit(X)
  assert nn.kneighbors(q)[1].shape == (7, 3)
  assert nn.kneighbors(q, n_neighbors=8)[1].shape == (7, 8) and nn.n_neighbors == 8  # the override sticks
  # one tile on one rank: one knn call, no combine
  be = backend.get()
  n0 = len(be.calls)
  NearestNeighbors(4).fit(expr.from_numpy(X, tile_hint=(120, 5))).kneighbors(q)
  assert be.calls[n0:].count('knn') == 1 and 'topk' not in be.calls[n0:]
  with pytest.raises(ValueError, match='121'):
    nn.kneighbors(q, n_neighbors=121)
  big = np.zeros((backend.KNN_K_MAX + 5, 2), np.float32)
  with pytest.raises(ValueError, match=str(backend.KNN_K_MAX)):
    NearestNeighbors(backend.KNN_K_MAX + 1).fit(big).kneighbors(big[:2])
  for bad in (0, -1, 2.5):
    with pytest.raises(ValueError):
      NearestNeighbors(bad).fit(X).kneighbors(q)
  with pytest.raises(ValueError):
    NearestNeighbors().fit(X).kneighbors(q[:, :3])
  with pytest.raises(ValueError):
    NearestNeighbors(algorithm='annoy')
  with pytest.raises(ValueError):
    NearestNeighbors().fit(X[0])


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
    from spartan_amd.examples.neighbors import NearestNeighbors
    from sort_ref import kat_ints
    from topk_ref import TopkFakeBackend, knn_data, knn_ref, same_bits, topk_ref
    backend.set_backend(TopkFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    ctx = runtime.get()
    assert ctx.world_size == world and ctx.dist_backend == 'gloo'
    a = kat_ints((40, 30), 11) % 13
    for hint in (None, (7, 30), (40, 8), (9, 11)):
      for axis in (0, 1):
        for largest in (False, True):
          x = expr.from_numpy(a, tile_hint=hint).force()
          want_v, want_i = topk_ref(a, 6, axis, largest)
          msg = '%s %s %s' % (hint, axis, largest)
          np.testing.assert_array_equal(expr.argtopk(x, 6, axis, largest).glom(), want_i, err_msg=msg)
          np.testing.assert_array_equal(expr.topk(x, 6, axis, largest).glom(), want_v, err_msg=msg)
    b = kat_ints((1000,), 12) % 9
    np.testing.assert_array_equal(expr.argtopk(expr.from_numpy(b, tile_hint=(37,)), 25).glom(), topk_ref(b, 25, 0)[1])
    X, qq = knn_data('grid', 150, 9, 4, np.float32, 2)
    s, want_i = knn_ref(X, qq, 7)
    for hint in (None, (40, 4), (40, 3)):  # X split over both ranks
      xd = expr.from_numpy(X, tile_hint=hint).force()
      if hint is not None:
        assert {ctx.owner(w) for w in xd.tiles.values()} == {0, 1}
      dist, ind = NearestNeighbors(7).fit(expr.lazify(xd)).kneighbors(qq)
      np.testing.assert_array_equal(ind, want_i, err_msg=str(hint))
      assert same_bits(dist, np.sqrt(s).astype(np.float32))
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


@needs_lib
@pytest.mark.parametrize('W', [2, 3])
def test_world2_gloo_topk(W):
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
def _lib():
  from spartan_amd import backend
  return backend.load_library()


@needs_lib
def test_topk_argument_validation_without_gpu():
  """Bad arguments are rejected before any device work (code + message).
  The pointers are host buffers: a call that got past its checks would try to
  launch on them, so every case here must stop at a check."""
  from spartan_amd import backend
  lib = _lib()
  bufs = [(ctypes.c_double * 16)() for _ in range(4)]
  p, v, i, pi = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
  EINVAL, ENOTSUP = -1, -3
  K, L = backend.TOPK_K_MAX, backend.SORT_LDS_MAX

  def call(dt, src, in_idx, ov, oi, geom, k, largest=0, ws=None, nbytes=0):
    return lib.spx_topk(dt, src, in_idx, ov, oi, geom[0], geom[1], geom[2], k, largest, ws, nbytes, None)

  assert call(99, p, None, v, i, (1, 4, 1), 1) == EINVAL and b'dtype' in lib.spx_last_error()
  for geom in ((-1, 4, 1), (1, -4, 1), (1, 4, -2), (2 ** 40, 2 ** 30, 2 ** 40)):
    assert call(3, p, None, v, i, geom, 1) == EINVAL and b'geometry' in lib.spx_last_error(), geom
  assert call(3, None, None, v, i, (1, 4, 1), 1) == EINVAL and b'null input' in lib.spx_last_error()
  assert call(3, p, None, None, None, (1, 4, 1), 1) == EINVAL and b'both null' in lib.spx_last_error()
  assert call(3, p, None, p, None, (1, 4, 1), 1) == EINVAL and b'alias' in lib.spx_last_error()
  assert call(2, p, None, None, p, (1, 4, 1), 1) == EINVAL and b'alias' in lib.spx_last_error()
  for k in (0, -3):
    assert call(3, p, pi, v, i, (1, 4, 1), k) == EINVAL and b'less than 1' in lib.spx_last_error()
  assert call(3, p, pi, v, i, (1, 4, 1), 5) == EINVAL and b'exceeds the line' in lib.spx_last_error()
  assert call(3, p, None, v, i, (1, 4 * K, 1), K + 1) == ENOTSUP and b'limit' in lib.spx_last_error()
  assert call(3, p, None, v, i, (1, 2 ** 31, 1), 1) == ENOTSUP and b'2^31' in lib.spx_last_error()
  # a select geometry without (or with too small a) workspace
  n = L + 1
  for want_idx, oi in ((0, None), (1, i)):
    need = lib.spx_topk_workspace(3, 1, n, 1, 4, want_idx)
    assert need > 0
    assert call(3, p, None, v, oi, (1, n, 1), 4) == EINVAL and b'workspace' in lib.spx_last_error()
    assert call(3, p, None, v, oi, (1, n, 1), 4, 1, p, need - 1) == EINVAL and b'workspace' in lib.spx_last_error()
  # zero lines: SPX_OK without a launch, whatever the pointers are
  for geom in ((0, 4, 1), (1, 4, 0), (0, 0, 5)):
    assert call(3, p, None, v, i, geom, 2) == 0, geom
    assert lib.spx_topk_workspace(3, geom[0], geom[1], geom[2], 2, 1) == 0
  assert lib.spx_topk_workspace(3, 5, L, 3, L, 1) == 0  # the LDS path needs none
  for bad in ((99, 1, 8, 1, 1), (3, -1, 8, 1, 1), (3, 1, 2 ** 31, 1, 1), (3, 2 ** 40, 2 ** 30, 2 ** 40, 1),
              (3, 1, 8, 1, 0), (3, 1, 8, 1, 9), (3, 1, 4 * K, 1, K + 1), (3, 1, 0, 1, 1)):
    assert lib.spx_topk_workspace(*bad, 0) < 0, bad
    assert lib.spx_topk_plan(*bad, None, None) < 0, bad


@needs_lib
def test_topk_plan_and_constants():
  from spartan_amd import backend
  lib = _lib()
  L = backend.SORT_LDS_MAX
  kmax, chunk = ctypes.c_int64(0), ctypes.c_int64(0)
  assert lib.spx_topk_plan(3, 1, 8, 1, 1, ctypes.byref(kmax), ctypes.byref(chunk)) == 0
  assert kmax.value == backend.TOPK_K_MAX == L and chunk.value > L and chunk.value % 256 == 0
  passes = {np.bool_: 1, np.int32: 4, np.float32: 4, np.int64: 8, np.float64: 8}
  for dt, want in passes.items():
    for inner in (1, 3):
      assert backend.topk_plan(5, L, inner, dt, 7) == ('lds', 0, chunk.value)
      assert backend.topk_plan(2, L + 1, inner, dt, L) == ('select', want, chunk.value)
  # a very long line is cut into a bounded number of chunks
  path, _p, big = backend.topk_plan(1, 2 ** 31 - 1, 1, np.float32, 10)
  assert path == 'select' and big > chunk.value and big % 256 == 0 and (2 ** 31 - 1 + big - 1) // big <= 1024
  with pytest.raises(ValueError):
    backend.topk_plan(1, 8, 1, np.float32, 9)
  # the workspace: per-chunk digit tables and k candidates per line, nothing of the line's size
  lines, n, k = 6, 3 * chunk.value + 9, 100
  need = lib.spx_topk_workspace(4, 2, n, 3, k, 1)
  assert lines * (4 * 1024 + k * 12) <= need <= lines * (4 * 1024 + k * 12) + (1 << 16)
  for name in ('spx_topk', 'spx_topk_workspace', 'spx_topk_plan', 'spx_knn', 'spx_knn_workspace', 'spx_knn_plan'):
    assert name in backend.EXPORTED


@needs_lib
def test_knn_argument_validation_without_gpu():
  from spartan_amd import backend
  lib = _lib()
  bufs = [(ctypes.c_double * 64)() for _ in range(5)]
  x, q, s, i, w = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
  EINVAL, ENOTSUP = -1, -3
  KM = backend.KNN_K_MAX
  assert KM >= 128

  def call(dt, Q, N, D, k, pts=x, ldp=None, qry=q, os_=s, oi=i, ws=w, nbytes=1 << 30):
    return lib.spx_knn(dt, Q, N, D, k, pts, D if ldp is None else ldp, qry, 0, os_, oi, ws, nbytes, None)

  for dt in (0, 1, 2, 99):
    assert call(dt, 2, 8, 2, 1) == ENOTSUP and b'F32/F64' in lib.spx_last_error()
  for Q, N, D in ((-1, 8, 2), (2, -8, 2), (2, 8, 0), (2, 8, -1)):
    assert call(3, Q, N, D, 1) == EINVAL and b'bad sizes' in lib.spx_last_error(), (Q, N, D)
  assert call(3, 2, 8, 4, 1, ldp=3) == EINVAL and b'bad sizes' in lib.spx_last_error()
  for k in (0, -2, 9):
    assert call(3, 2, 8, 2, k) == EINVAL and b'outside' in lib.spx_last_error(), k
  assert call(3, 2, 4 * KM, 2, KM + 1) == ENOTSUP and b'limit' in lib.spx_last_error()
  assert call(3, 2, 2 ** 31, 2, 1) == ENOTSUP and b'2^31' in lib.spx_last_error()
  for kw in (dict(pts=None), dict(qry=None), dict(os_=None), dict(oi=None)):
    assert call(3, 2, 8, 2, 1, **kw) == EINVAL and b'null' in lib.spx_last_error(), kw
  need = lib.spx_knn_workspace(3, 2, 8, 2, 3)
  assert need > 0
  assert call(3, 2, 8, 2, 3, ws=None, nbytes=0) == EINVAL and b'workspace' in lib.spx_last_error()
  assert call(3, 2, 8, 2, 3, nbytes=need - 1) == EINVAL and b'workspace' in lib.spx_last_error()
  assert call(3, 0, 8, 2, 3, ws=None, nbytes=0) == 0  # no queries: nothing runs
  for bad in ((2, 2, 8, 2, 1), (3, -1, 8, 2, 1), (3, 2, 8, 0, 1), (3, 2, 8, 2, 0), (3, 2, 8, 2, 9),
              (3, 2, 4 * KM, 2, KM + 1), (3, 2, 2 ** 31, 2, 1)):
    assert lib.spx_knn_workspace(*bad) < 0, bad
    assert lib.spx_knn_plan(*bad, None, None) < 0, bad
  # the plan: few queries cut the points into many ranges, many queries into few
  nch, chunk = backend.knn_plan(16, 2 ** 24, 16, 10)
  assert nch * chunk >= 2 ** 24 > (nch - 1) * chunk and nch >= 256 and chunk % 64 == 0
  nch2, chunk2 = backend.knn_plan(4096, 2 ** 20, 64, 10)
  assert nch2 * chunk2 >= 2 ** 20 and nch2 < nch
  assert backend.knn_plan(1, 100, 3, 5) == (1, backend.knn_plan(1, 1, 3, 1)[1])
  # the workspace holds the ranges' lists, never a (Q, N) matrix
  assert lib.spx_knn_workspace(3, 4096, 2 ** 20, 64, 10) < 4096 * 2 ** 20

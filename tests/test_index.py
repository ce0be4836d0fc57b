"""``spartan_amd.take`` / ``compress`` / ``a[i]`` host logic (no GPU): the
reference's KAT (tests/test_maptiles.py:47-56 there), NumPy's contract over
axes, virtual workers and tile layouts, the error and laziness rules,
composition, two gloo ranks, and the C-ABI argument checks of spx_take /
spx_compact_workspace / spx_compact_count / spx_compact.

The expression layer runs here over the CPU test double with NumPy kernels
(index_ref.IndexFakeBackend); the kernels themselves are tested on the GPU
in tests/test_index_gpu.py.
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
TEST_SIZE = 100


@pytest.fixture
def index_ctx(host_ctx):
  """host_ctx with the take / compact-capable test double installed."""
  from spartan_amd import backend
  from index_ref import IndexFakeBackend

  def make(num_workers=1):
    ctx = host_ctx(num_workers)
    backend.set_backend(IndexFakeBackend())
    return ctx
  return make


def _hints(shape):
  """The layouts of tests/test_sort.py::_hints: default, row strips, cuts
  along the last axis, blocks, (1, n, ...) and (..., n, 1) tiles."""
  nd = len(shape)
  return [None,
          tuple(2 if d == 0 else s for d, s in enumerate(shape)),
          tuple(3 if d == nd - 1 else s for d, s in enumerate(shape)),
          tuple(3 if d < 2 else s for d, s in enumerate(shape)),
          tuple(1 if d == 0 else s for d, s in enumerate(shape)),
          tuple(1 if d == nd - 1 else s for d, s in enumerate(shape))]


SHAPES = [(23,), (9, 7), (5, 6, 7), (4, 5, 3, 6)]


def _same(got, want, msg=''):
  from index_ref import bits
  assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape, msg)
  np.testing.assert_array_equal(bits(got), bits(want), err_msg=str(msg))


# ------------------------------------------------------------ reference KAT
@pytest.mark.parametrize('W', [1, 3])
def test_reference_kat_index_by_ones(index_ctx, W):
  index_ctx(W)
  from spartan_amd import expr
  a = expr.arange((TEST_SIZE, TEST_SIZE))
  b = expr.ones((10,), dtype=np.int64)
  z = a[b]
  val = expr.evaluate(z)
  assert val.shape == (10, TEST_SIZE)
  nx = np.arange(TEST_SIZE * TEST_SIZE).reshape(TEST_SIZE, TEST_SIZE)
  _same(val.glom(), nx[np.ones(10, np.int64)].astype(val.dtype))


# ------------------------------------------------------- NumPy's contract
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_take_every_axis_and_layout(index_ctx, W, shape):
  index_ctx(W)
  from spartan_amd import expr
  from index_ref import index_data, values
  a = values(shape, np.float64, 3)
  for hi, hint in enumerate(_hints(shape)):
    x = expr.from_numpy(a, tile_hint=hint)
    for axis in tuple(range(len(shape))) + (-1,):
      n = shape[axis]
      for ki, kind in enumerate(('random', 'negative', 'equal')):
        idx = index_data(n, (5, 1, 2 * n + 1)[ki], kind, 10 * hi + ki, (np.int64, np.int32)[ki % 2])
        e = expr.take(x, idx, axis)
        assert e.shape == np.take(a, idx, axis).shape and e.dtype == a.dtype
        _same(e.glom(), np.take(a, idx, axis), (hint, axis, kind))
    # a tiled index expression and a[i]
    idx = index_data(shape[0], 11, 'random', hi)
    _same(x[expr.from_numpy(idx, tile_hint=(4,))].glom(), a[idx], hint)


@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_compress_every_axis_and_layout(index_ctx, W, shape):
  index_ctx(W)
  from spartan_amd import expr
  from index_ref import mask_data, values
  a = values(shape, np.float32, 4)
  for hi, hint in enumerate(_hints(shape)):
    x = expr.from_numpy(a, tile_hint=hint)
    for axis in tuple(range(len(shape))) + (-1, None):
      n = a.size if axis is None else shape[axis]
      for kind in ('half', 'first', 'runs'):
        c = mask_data(n, kind, 7 + hi) != 0
        e = expr.compress(c, x, axis)
        got = e.glom()
        _same(got, np.compress(c, a, axis), (hint, axis, kind))
        assert e.shape == got.shape and e.dtype == a.dtype
    # a tiled condition expression, through a[i] with a 1-d mask of axis 0's length
    c = mask_data(shape[0], 'half', hi) != 0
    _same(x[expr.from_numpy(c, tile_hint=(4,))].glom(), a[c], hint)


@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_mask_of_the_arrays_shape(index_ctx, W, shape):
  index_ctx(W)
  from spartan_amd import expr
  from index_ref import mask_data, values
  a = values(shape, np.int64, 5)
  hints = _hints(shape)
  for hi, hint in enumerate(hints):
    x = expr.from_numpy(a, tile_hint=hint)
    for kind in ('half', 'sparse', 'all'):
      mk = (mask_data(a.size, kind, 20 + hi) != 0).reshape(shape)
      # the mask in the array's layout, in another layout, and as a lazy comparison
      for mh in (hint, hints[(hi + 2) % len(hints)]):
        _same(x[expr.from_numpy(mk, tile_hint=mh)].glom(), a[mk], (hint, mh, kind))
    _same(x[x > 0].glom(), a[a > 0], hint)


def test_edge_cases(index_ctx):
  index_ctx(3)
  from spartan_amd import expr
  from index_ref import values
  a = values((12, 5), np.float64, 6)
  for hint in (None, (5, 5), (12, 2)):
    x = expr.from_numpy(a, tile_hint=hint)
    # negative, duplicated, empty
    for idx in ([-1, -12, 0, 11, 3, 3, 3], []):
      for axis in (0, 1):
        ii = [i % 5 - (5 if i < 0 else 0) for i in idx] if axis else idx
        _same(expr.take(x, ii, axis).glom(), np.take(a, np.asarray(ii, np.int64), axis), (hint, axis))
    e = expr.take(x, [], 0)
    assert e.shape == (0, 5) and e.dtype == np.float64 and e.glom().shape == (0, 5)
    # other integer dtypes go through astype(int64)
    _same(expr.take(x, np.array([3, 250 % 12], np.uint8), 0).glom(), a[[3, 250 % 12]], hint)
    _same(expr.take(x, np.array([-2, 1], np.int16), 1).glom(), a[:, [-2, 1]], hint)
    # all-false and all-true masks
    none = np.zeros(12, bool)
    for axis, shape in ((0, (0, 5)), (None, (0,))):
      e = expr.compress(none[:5] if axis is None else none, x, axis)
      got = e.glom()
      assert got.shape == shape == e.shape and got.dtype == np.float64 == e.dtype
    got = x[expr.from_numpy(np.zeros((12, 5), bool))].glom()
    assert got.shape == (0,) and got.dtype == np.float64
    _same(expr.compress(np.ones(12, bool), x, 0).glom(), a, hint)
    _same(x[expr.from_numpy(np.ones((12, 5), bool))].glom(), a.reshape(-1), hint)
    # a non-bool condition goes through != 0; a short one drops the tail
    _same(expr.compress([0, 2, -1, 0, 0.5], x, 0).glom(), np.compress([0, 2, -1, 0, 0.5], a, 0), hint)
    _same(expr.compress([True, False, True], x, 1).glom(), np.compress([True, False, True], a, 1), hint)
    _same(expr.compress(np.arange(17) % 3 == 0, x).glom(), np.compress(np.arange(17) % 3 == 0, a), hint)
    # a longer one is fine while nothing past the end is true ...
    long_ok = np.r_[np.arange(12) % 2 == 0, np.zeros(4, bool)]
    _same(expr.compress(long_ok, x, 0).glom(), a[::2], hint)
    _same(expr.compress(np.r_[np.ones(60, bool), np.zeros(9, bool)], x).glom(), a.reshape(-1), hint)
    # ... and raises IndexError when forced otherwise, not before
    for cond, axis in ((np.r_[long_ok, True], 0), (np.ones(61, bool), None), (np.ones(6, bool), 1)):
      e = expr.compress(cond, x, axis)
      with pytest.raises(IndexError):
        e.force()
  x1 = expr.from_numpy(np.arange(20.0), tile_hint=(6,))
  for bad in ([0, 20], [-21, 3], [5, 7, 1 << 40]):
    e = expr.take(x1, bad)  # building the node raises nothing
    assert e.shape == (len(bad),)
    with pytest.raises(IndexError):
      e.glom()
  e = x[expr.from_numpy(np.array([0, 12]))]
  with pytest.raises(IndexError):
    e.force()


def test_shape_dtype_laziness_and_validation(index_ctx):
  index_ctx(2)
  import spartan_amd
  from spartan_amd import backend, expr
  from spartan_amd.expr.filter import FilterExpr
  assert spartan_amd.take is expr.take and spartan_amd.compress is expr.compress
  a = (np.arange(1200, dtype=np.int32).reshape(40, 30) * 7919) % 173
  x = expr.from_numpy(a, tile_hint=(9, 11))
  be = backend.get()
  n0 = len(be.calls)
  i = expr.from_numpy(np.array([3, -1, 3]))
  t = expr.take(x * 2, i, axis=1)
  g = x[i]
  kx = expr.from_numpy(np.arange(40) % 9, tile_hint=(7,))
  c = expr.compress(kx > 5, x, axis=0)
  m = x[x > 100]
  for e in (t, g, c, m):
    assert isinstance(e, FilterExpr) and isinstance(e, expr.Expr) and e.dtype == np.int32
  assert t.shape == (40, 3) and g.shape == (3, 30)  # known without evaluation
  assert len(be.calls) == n0 and all(e.cache() is None for e in (t, g, c, m))  # nothing ran
  with pytest.raises(expr.NotShapeable):
    c.compute_shape()
  with pytest.raises(expr.NotShapeable):
    m.compute_shape()
  keep = np.arange(40) % 9 > 5
  assert c.shape == (int(keep.sum()), 30) and c.cache() is not None  # .shape forced it
  _same(c.glom(), a[keep])
  assert m.shape == (int((a > 100).sum()),)
  _same(t.glom(), (a * 2)[:, [3, -1, 3]])
  # validation
  for bad in (2, -3, 1.5, 'x'):
    with pytest.raises(ValueError):
      expr.take(x, [0], axis=bad)
    with pytest.raises(ValueError):
      expr.compress([True], x, axis=bad)
  with pytest.raises(NotImplementedError):
    expr.take(x, [[0, 1], [2, 3]])
  with pytest.raises(NotImplementedError):
    x[expr.from_numpy(np.zeros((2, 2), np.int64))]
  with pytest.raises(IndexError):
    expr.take(x, [0.5, 1.0])
  with pytest.raises(ValueError):
    expr.compress(np.ones((2, 2), bool), x)
  for shape in ((40, 29), (30,), (40, 30, 1)):
    with pytest.raises(IndexError):
      x[expr.from_numpy(np.ones(shape, bool))]
  # a raw host array or list inside [] stays refused, as does an index inside a tuple
  for raw in (np.array([1, 2]), [1, 2], np.ones(40, bool)):
    with pytest.raises(NotImplementedError):
      x[raw]
  with pytest.raises(NotImplementedError):
    x[i, 0]


@pytest.mark.parametrize('W', [1, 3])
def test_composition(index_ctx, W):
  index_ctx(W)
  from spartan_amd import expr
  from index_ref import values
  r = np.random.RandomState(8)
  a = r.rand(37, 6)
  k = r.randint(0, 9, 37).astype(np.int64)
  x = expr.from_numpy(a, tile_hint=(8, 6))
  kx = expr.from_numpy(k, tile_hint=(10,))
  _same(x[expr.argsort(kx)].glom(), a[np.argsort(k, kind='stable')])
  _same(x[x > 0.5].glom(), a[a > 0.5])
  i = expr.from_numpy(np.array([5, 0, -1, 5]))
  e = (expr.take(x * 2, i) + 1)
  _same(e.optimized().glom(), np.take(a * 2, [5, 0, -1, 5], 0) + 1)
  _same((expr.compress(kx > 3, x * 2, axis=0) + 1).optimized().glom(), (a * 2)[k > 3] + 1)
  # labels pick rows; a lazy child and a lazy parent of the node
  labels = expr.argmin(x, axis=1)
  centres = expr.from_numpy(values((6, 4), np.float64, 2))
  _same(expr.take(centres, labels).glom(), values((6, 4), np.float64, 2)[np.argmin(a, axis=1)])
  # (a sum over uneven output tiles: the addition order is the tiles', so not bit for bit)
  np.testing.assert_allclose(expr.sum(x[kx == 2], axis=0).glom(), a[k == 2].sum(axis=0), rtol=1e-13)
  # views, host arrays and maps over them (replicated inputs)
  v = a[3:29, 1:5].T
  _same(expr.take(x[3:29, 1:5].T, [0, -1], 1).glom(), v[:, [0, -1]])
  _same(expr.compress(v[0] > 0.5, x[3:29, 1:5].T, 1).glom(), v[:, v[0] > 0.5])
  y = x[3:29, 1:5].T
  _same(y[y > 0.5].glom(), v[v > 0.5])
  for src in (a, expr.as_array(a) * 2):
    want = a if src is a else a * 2
    res = expr.take(src, [4, 4, -1], 1).force()
    _same(res.glom(), want[:, [4, 4, -1]])
    _same(expr.compress(k > 3, src, 0).glom(), want[k > 3])
    _same(expr.compress(np.arange(50) % 7 == 0, src).glom(), np.compress(np.arange(50) % 7 == 0, want))
  from spartan_amd.array.distarray import ReplicatedArray
  assert isinstance(expr.take(expr.as_array(a) * 2, [1], 0).force(), ReplicatedArray)
  assert isinstance(expr.compress(k > 3, expr.as_array(a) * 2, 0).force(), ReplicatedArray)


def test_bits_and_dtypes(index_ctx):
  """-0.0, NaN payloads, bool bytes and the full integer range arrive
  unchanged through both take routes and both compaction routes."""
  index_ctx(3)
  from spartan_amd import expr
  from index_ref import index_data, mask_data, values
  for dt in (np.bool_, np.int32, np.int64, np.float32, np.float64):
    a = values((31, 9), dt, 12)
    idx = index_data(31, 50, 'random', 3)
    c = mask_data(31, 'half', 4) != 0
    mk = (mask_data(31 * 9, 'half', 5) != 0).reshape(31, 9)
    for hint in ((7, 9), (31, 4), (7, 4)):
      x = expr.from_numpy(a, tile_hint=hint)
      _same(x[expr.from_numpy(idx)].glom(), a[idx], (dt, hint))
      _same(expr.take(x, idx[:9] % 9, 1).glom(), a[:, idx[:9] % 9], (dt, hint))
      _same(expr.compress(c, x, 0).glom(), a[c], (dt, hint))
      _same(x[expr.from_numpy(mk)].glom(), a[mk], (dt, hint))
  with pytest.raises(TypeError):
    expr.take(np.ones((4, 5), np.complex128), [0]).glom()


def test_plan_replay(index_ctx):
  index_ctx(3)
  from spartan_amd import expr
  from spartan_amd.expr import plan_cache
  a = np.random.RandomState(1).rand(40, 30)
  X = expr.lazify(expr.from_numpy(a, tile_hint=(9, 30)).force())
  I = expr.lazify(expr.from_numpy(np.array([7, 7, -2, 39])).force())
  plan_cache.clear()
  h0, m0 = plan_cache.STATS['hits'], plan_cache.STATS['misses']
  r1 = (expr.take(X * 2, I, 0) + 1).optimized().glom()
  assert plan_cache.STATS['misses'] == m0 + 1
  r2 = (expr.take(X * 2, I, 0) + 1).optimized().glom()
  assert plan_cache.STATS['hits'] == h0 + 1
  _same(r1, r2)
  _same(r1, (a * 2)[[7, 7, -2, 39]] + 1)
  J = expr.lazify(expr.from_numpy(np.array([7, 7, -2, 29])).force())
  r3 = (expr.take(X * 2, J, 1) + 1).optimized().glom()  # another axis is another structure
  assert plan_cache.STATS['misses'] == m0 + 2
  _same(r3, np.take(a * 2, [7, 7, -2, 29], 1) + 1)
  r4 = (expr.compress(X.sum(axis=1) > 15, X * 2, 0) + 1).optimized().glom()
  r5 = (expr.compress(X.sum(axis=1) > 15, X * 2, 0) + 1).optimized().glom()
  _same(r4, r5)
  _same(r4, (a * 2)[a.sum(axis=1) > 15] + 1)


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
    from index_ref import IndexFakeBackend, bits, index_data, mask_data, values
    backend.set_backend(IndexFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    ctx = runtime.get()
    assert ctx.world_size == world and ctx.dist_backend == 'gloo'

    def same(got, want, msg):
      assert got.dtype == want.dtype and got.shape == want.shape, msg
      np.testing.assert_array_equal(bits(got), bits(want), err_msg=str(msg))

    for dt in (np.float64, np.bool_):
      a = values((40, 30), dt, 11)
      idx = index_data(40, 70, 'random', 1)
      c0 = mask_data(40, 'half', 2) != 0
      mk = (mask_data(1200, 'half', 3) != 0).reshape(40, 30)
      for hint in (None, (7, 30), (40, 8), (9, 11), (40, 30)):
        x = expr.lazify(expr.from_numpy(a, tile_hint=hint).force())
        same(expr.take(x, idx, 0).glom(), a[idx], (hint, 'take0'))
        same(expr.take(x, idx[:11] % 30, 1).glom(), a[:, idx[:11] % 30], (hint, 'take1'))
        same(x[expr.from_numpy(idx, tile_hint=(9,))].glom(), a[idx], (hint, 'getitem'))
        same(expr.compress(c0, x, 0).glom(), a[c0], (hint, 'compress0'))
        same(expr.compress(c0[:30], x, 1).glom(), a[:, c0[:30]], (hint, 'compress1'))
        same(expr.compress(mk.reshape(-1)[:700], x).glom(), np.compress(mk.reshape(-1)[:700], a), (hint, 'flat'))
        same(x[expr.from_numpy(mk, tile_hint=(9, 11))].glom(), a[mk], (hint, 'mask'))
        for bad in (expr.take(x, [0, 40], 0), expr.take(x, [-31], 1), expr.compress(np.ones(41, bool), x, 0)):
          try:  # every rank raises: nobody is left waiting in a collective
            bad.force()
            raise AssertionError('no IndexError')
          except IndexError:
            pass
    a = values((40, 30), np.float64, 11)
    x = expr.from_numpy(a, tile_hint=(9, 11))
    k = expr.from_numpy(np.arange(40) * 7 % 11, tile_hint=(9,))
    same(x[expr.argsort(k)].glom(), a[np.argsort(np.arange(40) * 7 % 11, kind='stable')], 'argsort')
    same((expr.take(x + x, [3, 3], 0) + 1).optimized().glom(), (a + a)[[3, 3]] + 1, 'lazy')
    assert expr.compress(np.zeros(40, bool), x, 0).glom().shape == (0, 30)
    # a single tile on rank 0: rank 1 owns nothing and still takes part
    y = expr.from_numpy(a[:5], tile_hint=(5, 30))
    same(expr.take(y, [4, 0], 0).glom(), a[[4, 0]], 'one tile')
    same(y[y > 0].glom(), a[:5][a[:5] > 0], 'one tile mask')
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
def test_world2_gloo_index(W):
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
def _index_lib():
  from spartan_amd import backend
  lib = backend.load_library()
  return lib


@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_index_argument_validation_without_gpu():
  """Bad arguments are rejected before any device work (code + message), and
  empty work is SPX_OK without a launch.  The pointers are host buffers: a
  call that got past its checks would try to launch on them, so every case
  here must stop at a check."""
  from spartan_amd import backend
  lib = _index_lib()
  bufs = [(ctypes.c_double * 64)() for _ in range(4)]
  p, i, o, e = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
  EINVAL = -1
  err = lambda: lib.spx_last_error()

  def take(dt=3, it=2, src=p, idx=i, out=o, outer=1, n_total=8, lo=0, n_local=8, m=4, inner=1, oos=4, ors=1, er=e):
    return lib.spx_take(dt, it, src, idx, out, outer, n_total, lo, n_local, m, inner, oos, ors, er, None)
  assert take(dt=99) == EINVAL and b'dtype' in err()
  assert take(it=3) == EINVAL and b'index dtype' in err()
  assert take(it=0) == EINVAL and b'index dtype' in err()
  for kw in (dict(outer=-1), dict(n_total=-8), dict(lo=-1), dict(n_local=-1), dict(m=-4), dict(inner=-1),
             dict(lo=1), dict(n_local=9), dict(outer=2 ** 40, m=2 ** 30, inner=2 ** 40)):
    assert take(**kw) == EINVAL and b'geometry' in err(), kw
  for kw in (dict(inner=2, ors=1), dict(oos=-1), dict(ors=-1)):
    assert take(**kw) == EINVAL and b'strides' in err(), kw
  for kw in (dict(src=None), dict(idx=None), dict(out=None), dict(er=None)):
    assert take(**kw) == EINVAL and b'null' in err(), kw
  for kw in (dict(outer=0), dict(m=0), dict(inner=0, ors=0)):
    assert take(**kw) == 0, kw

  T = backend.COMPACT_TILE
  ws = lib.spx_compact_workspace
  assert T >= 256 and T % 256 == 0
  assert ws(0) == 0 and ws(1) == 8 and ws(T) == 8 and ws(T + 1) == 16 and ws(5 * T) == 40
  assert ws(-1) < 0 and ws(2 ** 61) < 0
  assert ws(2 ** 33) >= 8 * (2 ** 33 // T)
  need = ws(3 * T)
  assert lib.spx_compact_count(p, -1, o, e, 64, None) == EINVAL and b'length' in err()
  assert lib.spx_compact_count(p, 8, None, e, 64, None) == EINVAL and b'total' in err()
  assert lib.spx_compact_count(None, 8, o, e, 64, None) == EINVAL and b'mask' in err()
  assert lib.spx_compact_count(p, 3 * T, o, None, 0, None) == EINVAL and b'workspace' in err()
  assert lib.spx_compact_count(p, 3 * T, o, e, need - 1, None) == EINVAL and b'workspace' in err()
  assert lib.spx_compact_count(p, 8, o, ctypes.c_void_p(e.value + 4), 64, None) == EINVAL and b'aligned' in err()

  def compact(dt=3, src=p, mask=i, out=o, outer=1, n=8, inner=1, count=4, w=e, nb=64):
    return lib.spx_compact(dt, src, mask, out, outer, n, inner, count, w, nb, None)
  assert compact(dt=7) == EINVAL and b'dtype' in err()
  for kw in (dict(outer=-1), dict(n=-8), dict(inner=-1), dict(count=-1), dict(count=9),
             dict(outer=2 ** 40, n=2 ** 30, inner=2 ** 40, count=1)):
    assert compact(**kw) == EINVAL and b'geometry' in err(), kw
  for kw in (dict(src=None), dict(mask=None), dict(out=None)):
    assert compact(**kw) == EINVAL and b'null' in err(), kw
  assert compact(w=None, nb=0) == EINVAL and b'workspace' in err()
  assert compact(n=3 * T, w=e, nb=need - 1) == EINVAL and b'workspace' in err()
  assert compact(w=ctypes.c_void_p(e.value + 4)) == EINVAL and b'aligned' in err()
  for kw in (dict(outer=0), dict(n=0, count=0), dict(inner=0), dict(count=0)):
    assert compact(**kw) == 0, kw
  for name in ('spx_take', 'spx_compact_workspace', 'spx_compact_count', 'spx_compact'):
    assert name in backend.EXPORTED

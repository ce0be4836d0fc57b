"""``spartan_amd.expr.stencil`` host logic (no GPU): the reference's three
convnet drivers restated (tests/test_stencil.py, tests/test_convnet.py and
tests/benchmark_convnet.py there), both functions over tile layouts, filter
kinds, replicated inputs, composition, plan replay, laziness and the
build-time errors, an empty N, two gloo ranks, and the C-ABI argument checks
of spx_stencil_plan / spx_stencil / spx_maxpool.

The expression layer runs here over the CPU test double with NumPy kernels
(stencil_ref.StencilFakeBackend); the kernels themselves are tested on the GPU
in tests/test_stencil_gpu.py.
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
def stencil_ctx(host_ctx):
  """host_ctx with the stencil / maxpool-capable test double installed."""
  from spartan_amd import backend
  from stencil_ref import StencilFakeBackend

  def make(num_workers=1):
    ctx = host_ctx(num_workers)
    backend.set_backend(StencilFakeBackend())
    return ctx
  return make


def _eq(got, want, msg=''):
  assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape, msg)
  np.testing.assert_array_equal(got, want, err_msg=str(msg))


# ------------------------------------------------- the reference's drivers
@pytest.mark.parametrize('W', [1, 4])
def test_reference_drivers(stencil_ctx, W):
  stencil_ctx(W)
  from spartan_amd import expr
  from spartan_amd.expr import stencil
  from stencil_ref import (convnet_ref, driver_benchmark, driver_test_convnet, driver_test_stencil, int_data,
                           stencil_ref)
  res, a, f = driver_test_stencil(expr, stencil, W)
  assert res.shape == (8, 32) + a.shape[2:] and res.dtype == np.float64
  _eq(res.glom(), stencil_ref(a, f), 'test_stencil')
  ints = lambda shape, seed: int_data(shape, np.float64, seed)
  for data in (None, ints):
    res, a, ws = driver_test_convnet(expr, stencil, W, data=data)
    assert res.shape == (1, 1, 2, 2)
    _eq(res.glom(), convnet_ref(a, ws), 'test_convnet')
    res, a, ws = driver_benchmark(expr, stencil, W, data=data)
    assert res.shape == (8, 4, 2, 2)
    _eq(res.glom(), convnet_ref(a, ws), 'benchmark_convnet')


# ----------------------------------------------------------------- layouts
@pytest.mark.parametrize('W', [1, 4])
def test_stencil_and_maxpool_over_layouts(stencil_ctx, W):
  stencil_ctx(W)
  from spartan_amd import expr
  from spartan_amd.expr import stencil
  from stencil_ref import int_data, layouts, maxpool_ref, pool_data, stencil_ref
  shape = (5, 4, 7, 9)
  a = int_data(shape, np.float64, 1)
  f = int_data((3, 4, 3, 2), np.float64, 2)
  want = stencil_ref(a, f)
  b = pool_data(shape, np.int32, 3)
  for hint in layouts(shape):
    x = expr.from_numpy(a, tile_hint=hint)
    e = stencil.stencil(x, f)
    assert e.shape == (5, 3, 7, 9) and e.dtype == np.float64
    val = e.force()
    _eq(val.glom(), want, hint)
    if hint is not None:  # the output is cut along axis 0 at the input's cuts and nowhere else
      cuts = sorted({(t.ul[0], t.lr[0]) for t in x.force().tiles})
      assert sorted((t.ul[0], t.lr[0]) for t in val.tiles) == cuts
      assert all(t.ul[1:] == (0, 0, 0) and t.lr[1:] == (3, 7, 9) for t in val.tiles)
    y = expr.from_numpy(b, tile_hint=hint)
    for pool, stride in ((2, 2), (3, 2), (2, 3), (1, 1), (9, 4)):
      m = stencil.maxpool(y, pool, stride)
      assert m.shape == (5, 4, -(-7 // stride), -(-9 // stride)) and m.dtype == np.int32
      _eq(m.glom(), maxpool_ref(b, pool, stride), (hint, pool, stride))


def test_filter_kinds_and_replicated_inputs(stencil_ctx):
  stencil_ctx(3)
  from spartan_amd import expr
  from spartan_amd.array.distarray import ReplicatedArray
  from spartan_amd.expr import stencil
  from stencil_ref import int_data, maxpool_ref, stencil_ref
  a = int_data((4, 2, 6, 5), np.float32, 4)
  f = int_data((3, 2, 2, 4), np.float32, 5)
  want = stencil_ref(a, f).astype(np.float32)
  x = expr.from_numpy(a, tile_hint=(2, 2, 3, 5))
  kinds = [f,                                           # a NumPy array
           expr.from_numpy(f, tile_hint=(2, 1, 2, 2)).force(),  # an array, in tiles
           expr.from_numpy(f, tile_hint=(2, 1, 2, 2)),  # an expression
           expr.from_numpy(f) * 1,                      # a lazy expression
           expr.as_array(f) * 1]                        # a replicated value
  for k, flt in enumerate(kinds):
    _eq(stencil.stencil(x, flt).glom(), want, k)
  # replicated / host images give a replicated result
  for src in (a, expr.as_array(a) * 1):
    val = stencil.stencil(src, f).force()
    assert isinstance(val, ReplicatedArray)
    _eq(val.glom(), want)
    val = stencil.maxpool(src, 3, 2).force()
    assert isinstance(val, ReplicatedArray)
    _eq(val.glom(), maxpool_ref(a, 3, 2))
  # stride is accepted and ignored
  _eq(stencil.stencil(x, f, 2).glom(), want)
  _eq(stencil.stencil(x, f, stride=7).glom(), want)


@pytest.mark.parametrize('W', [1, 4])
def test_composition(stencil_ctx, W):
  stencil_ctx(W)
  from spartan_amd import expr
  from spartan_amd.expr import stencil
  from stencil_ref import int_data, maxpool_ref, stencil_ref
  a = int_data((6, 3, 8, 8), np.float64, 6)
  f = int_data((2, 3, 3, 3), np.float64, 7)
  x = expr.from_numpy(a, tile_hint=(2, 3, 8, 8))
  fx = expr.from_numpy(f)
  # map below and above, .optimized()
  e = stencil.stencil(x * 2, fx + 1) + 1
  _eq(e.optimized().glom(), stencil_ref(a * 2, f + 1) + 1)
  m = stencil.maxpool(x * 2 - 1, 2, 2) * 3
  _eq(m.optimized().glom(), maxpool_ref(a * 2 - 1, 2, 2) * 3)
  # slice views as input (spatial and batch cuts) and of the result
  v = a[1:5, :, 2:7, 1:8]
  _eq(stencil.stencil(x[1:5, :, 2:7, 1:8], fx).glom(), stencil_ref(v, f))
  _eq(stencil.maxpool(x[1:5, :, 2:7, 1:8], 3, 2).glom(), maxpool_ref(v, 3, 2))
  _eq(stencil.stencil(x, fx)[2:4, 1:2].glom(), stencil_ref(a, f)[2:4, 1:2])
  # a reduction over the result
  conv = stencil_ref(a, f)
  _eq(expr.sum(stencil.stencil(x, fx), axis=0).glom(), conv.sum(axis=0))
  np.testing.assert_array_equal(expr.sum(stencil.maxpool(stencil.stencil(x, fx))).glom(),
                                maxpool_ref(conv, 2, 2).sum())


def test_plan_replay(stencil_ctx):
  stencil_ctx(3)
  from spartan_amd import expr
  from spartan_amd.expr import plan_cache, stencil
  from stencil_ref import int_data, maxpool_ref, stencil_ref
  a = int_data((6, 2, 5, 5), np.float64, 8)
  f = int_data((3, 2, 2, 2), np.float64, 9)
  X = expr.lazify(expr.from_numpy(a, tile_hint=(2, 2, 5, 5)).force())
  Fx = expr.lazify(expr.from_numpy(f).force())
  build = lambda p, s: (stencil.maxpool(stencil.stencil(X * 2, Fx), p, s) + 1).optimized().glom()
  plan_cache.clear()
  h0, m0 = plan_cache.STATS['hits'], plan_cache.STATS['misses']
  r1 = build(2, 2)
  assert plan_cache.STATS['misses'] == m0 + 1
  r2 = build(2, 2)
  assert plan_cache.STATS['hits'] == h0 + 1
  _eq(r1, r2)
  _eq(r1, maxpool_ref(stencil_ref(a * 2, f), 2, 2) + 1)
  r3 = build(3, 2)  # another window is another structure
  assert plan_cache.STATS['misses'] == m0 + 2
  _eq(r3, maxpool_ref(stencil_ref(a * 2, f), 3, 2) + 1)


def test_laziness_and_build_time_errors(stencil_ctx):
  stencil_ctx(2)
  from spartan_amd import backend, expr
  from spartan_amd.expr import stencil
  from spartan_amd.expr.stencil import MaxpoolExpr, StencilExpr
  import spartan_amd.expr
  assert not callable(getattr(spartan_amd.expr, 'stencil'))  # the submodule, not a function
  a = np.ones((4, 3, 6, 6), np.float32)
  x = expr.from_numpy(a, tile_hint=(2, 3, 6, 6))
  f = expr.from_numpy(np.ones((5, 3, 2, 2), np.float32))
  be = backend.get()
  n0 = len(be.calls)
  c = stencil.stencil(x * 2, f, 2)
  p = stencil.maxpool(c)
  assert isinstance(c, StencilExpr) and isinstance(p, MaxpoolExpr) and isinstance(p, expr.Expr)
  assert c.shape == (4, 5, 6, 6) and p.shape == (4, 5, 3, 3) and c.dtype == np.float32 == p.dtype
  assert len(be.calls) == n0 and c.cache() is None and p.cache() is None  # nothing ran
  assert p.glom().shape == (4, 5, 3, 3)
  assert 'stencil' in be.calls and 'maxpool' in be.calls
  # dtypes: float32 / float64 only, and one dtype for both
  for bad in (np.int32, np.int64, np.bool_, np.float16, np.complex128):
    with pytest.raises(TypeError, match=np.dtype(bad).name):
      stencil.stencil(np.ones((1, 3, 4, 4), bad), np.ones((1, 3, 2, 2), np.float32))
    with pytest.raises(TypeError, match=np.dtype(bad).name):
      stencil.stencil(x, np.ones((1, 3, 2, 2), bad))
  with pytest.raises(TypeError):
    stencil.stencil(x, np.ones((1, 3, 2, 2), np.float64))
  # shapes
  for bad_images, bad_filters in ((np.ones((3, 6, 6), np.float32), f), (x, np.ones((3, 2, 2), np.float32)),
                                  (np.ones((1, 4, 3, 6, 6), np.float32), f)):
    with pytest.raises(ValueError):
      stencil.stencil(bad_images, bad_filters)
  with pytest.raises(ValueError, match='channels'):
    stencil.stencil(x, np.ones((5, 2, 2, 2), np.float32))
  for shape in ((0, 3, 2, 2), (5, 3, 0, 2), (5, 3, 2, 0)):
    with pytest.raises(ValueError):
      stencil.stencil(x, np.ones(shape, np.float32))
  # maxpool
  for kw in (dict(pool_size=0), dict(stride=0), dict(pool_size=-1), dict(stride=-2), dict(pool_size=1.5)):
    with pytest.raises(ValueError):
      stencil.maxpool(x, **kw)
  with pytest.raises(ValueError):
    stencil.maxpool(np.ones((3, 6, 6), np.float32))
  with pytest.raises(TypeError):
    stencil.maxpool(np.ones((1, 1, 4, 4), np.complex128))
  for dt in (np.bool_, np.int32, np.int64, np.float32, np.float64):
    assert stencil.maxpool(np.ones((1, 1, 4, 4), dt)).dtype == dt
  assert len(be.calls) > n0


def test_maxpool_values(stencil_ctx):
  """NaN and infinities, every dtype, windows smaller and larger than the stride."""
  stencil_ctx(3)
  from spartan_amd import expr
  from spartan_amd.expr import stencil
  from stencil_ref import maxpool_ref, pool_data
  for dt in (np.bool_, np.int32, np.int64, np.float32, np.float64):
    a = pool_data((3, 2, 7, 5), dt, 11)
    if np.dtype(dt).kind == 'f':
      a[0, 0, 1, 1] = np.nan
      a[1, 1, 6, 4] = np.nan
      a[2, 0, 0, 0] = np.inf
      a[2, 1, :, :] = -np.inf
    for hint in (None, (1, 2, 7, 5), (3, 2, 4, 3)):
      x = expr.from_numpy(a, tile_hint=hint)
      for pool, stride in ((2, 2), (1, 2), (3, 1), (4, 3)):
        _eq(stencil.maxpool(x, pool, stride).glom(), maxpool_ref(a, pool, stride), (dt, hint, pool, stride))
  got = stencil.maxpool(np.array([[[[-np.inf, np.nan], [1.0, 2.0]]]]), 2, 2).glom()
  assert got.shape == (1, 1, 1, 1) and np.isnan(got).all()


def test_empty_n(stencil_ctx):
  stencil_ctx(2)
  from spartan_amd import backend, expr
  from spartan_amd.expr import stencil
  be = backend.get()
  n0 = len(be.calls)
  e = stencil.stencil(np.empty((0, 3, 6, 6), np.float32), np.ones((5, 3, 2, 2), np.float32))
  assert e.shape == (0, 5, 6, 6) and e.dtype == np.float32
  got = e.glom()
  assert isinstance(got, np.ndarray) and got.shape == (0, 5, 6, 6) and got.dtype == np.float32
  m = stencil.maxpool(np.empty((0, 3, 6, 5), np.int64), 2, 2)
  assert m.shape == (0, 3, 3, 3)
  got = m.glom()
  assert got.shape == (0, 3, 3, 3) and got.dtype == np.int64
  chained = stencil.maxpool(stencil.stencil(np.empty((0, 3, 6, 6)), np.ones((5, 3, 2, 2))))
  assert chained.glom().shape == (0, 5, 3, 3)
  assert 'stencil' not in be.calls[n0:] and 'maxpool' not in be.calls[n0:]


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
    from spartan_amd.expr import stencil
    from stencil_ref import StencilFakeBackend, int_data, layouts, maxpool_ref, stencil_ref
    backend.set_backend(StencilFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    ctx = runtime.get()
    assert ctx.world_size == world and ctx.dist_backend == 'gloo'

    def same(got, want, msg):
      assert got.dtype == want.dtype and got.shape == want.shape, msg
      np.testing.assert_array_equal(got, want, err_msg=str(msg))

    shape = (5, 4, 7, 9)
    a = int_data(shape, np.float64, 1)
    f = int_data((3, 4, 3, 2), np.float64, 2)
    conv = stencil_ref(a, f)
    for hint in layouts(shape) + [(5, 4, 7, 9)]:  # per-owner, gathered slabs, and one tile on rank 0
      x = expr.lazify(expr.from_numpy(a, tile_hint=hint).force())
      for flt in (f, expr.from_numpy(f, tile_hint=(2, 2, 3, 2))):
        same(stencil.stencil(x, flt).glom(), conv, (hint, 'stencil'))
      same(stencil.maxpool(x, 3, 2).glom(), maxpool_ref(a, 3, 2), (hint, 'maxpool'))
      e = stencil.maxpool(stencil.stencil(x * 2, f, 2)) + 1
      same(e.optimized().glom(), maxpool_ref(conv * 2, 2, 2) + 1, (hint, 'chain'))
    same(stencil.stencil(a, f).glom(), conv, 'replicated')
    assert stencil.stencil(np.empty((0, 4, 7, 9)), f).glom().shape == (0, 3, 7, 9)
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
def test_world2_gloo_stencil(W):
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
@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_stencil_argument_validation_without_gpu():
  """Bad arguments are rejected before any device work (code + message), and
  N == 0 is SPX_OK without a launch.  The pointers are host buffers: a call
  that got past its checks would try to launch on them, so every case here
  must stop at a check."""
  from spartan_amd import backend
  lib = backend.load_library()
  bufs = [(ctypes.c_double * 64)() for _ in range(3)]
  p, f, o = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
  EINVAL, ENOTSUP = -1, -3
  err = lambda: lib.spx_last_error()

  for dt, name in ((3, np.float32), (4, np.float64)):
    bm, bn, bk = backend.stencil_plan(name)
    assert bm >= 16 and bn >= 64 and bk >= 4 and bn % 64 == 0
    v = ctypes.c_int64(0)
    assert lib.spx_stencil_plan(dt, None, ctypes.byref(v), None) == 0 and v.value == bn
  assert lib.spx_stencil_plan(1, None, None, None) == EINVAL and b'dtype' in err()
  assert lib.spx_stencil_plan(9, None, None, None) == EINVAL and b'dtype' in err()
  with pytest.raises(TypeError):
    backend.stencil_plan(np.int32)

  def conv(dt=3, img=p, flt=f, out=o, N=1, C=1, W=2, H=2, F=1, fw=1, fh=1):
    return lib.spx_stencil(dt, img, flt, out, N, C, W, H, F, fw, fh, None)
  for dt in (0, 1, 2, 7, -1):
    assert conv(dt=dt) == EINVAL and b'dtype' in err(), dt
  for kw in (dict(N=-1), dict(C=0), dict(W=0), dict(H=0), dict(F=0), dict(fw=0), dict(fh=0), dict(C=-3),
             dict(W=-1), dict(H=-2), dict(F=-1), dict(fw=-1), dict(fh=-5)):
    assert conv(**kw) == EINVAL and b'extent' in err(), kw
  for kw in (dict(img=None), dict(flt=None), dict(out=None)):
    assert conv(**kw) == EINVAL and b'null' in err(), kw
  for kw in (dict(W=2 ** 16, H=2 ** 15), dict(W=2 ** 31), dict(H=2 ** 40), dict(C=2 ** 20, W=2 ** 6, H=2 ** 6),
             dict(F=2 ** 20, W=2 ** 6, H=2 ** 6), dict(F=2 ** 16, C=2 ** 8, fw=2 ** 4, fh=2 ** 4),
             dict(fw=2 ** 20, H=2 ** 12), dict(fw=2 ** 62, fh=4), dict(N=2 ** 62, W=2 ** 10, H=2 ** 10)):
    assert conv(**kw) == ENOTSUP and b'overflow' in err(), kw
  assert conv(N=0) == 0 and conv(N=0, img=None, flt=None, out=None) == 0

  def pool(dt=3, src=p, out=o, NC=1, W=2, H=2, pl=2, st=2):
    return lib.spx_maxpool(dt, src, out, NC, W, H, pl, st, None)
  for dt in (5, 9, -1):
    assert pool(dt=dt) == EINVAL and b'dtype' in err(), dt
  for kw in (dict(NC=-1), dict(W=0), dict(H=0), dict(W=-2), dict(H=-1)):
    assert pool(**kw) == EINVAL and b'extent' in err(), kw
  for kw in (dict(pl=0), dict(st=0), dict(pl=-1), dict(st=-3)):
    assert pool(**kw) == EINVAL and b'window' in err(), kw
  for kw in (dict(src=None), dict(out=None)):
    assert pool(**kw) == EINVAL and b'null' in err(), kw
  for kw in (dict(W=2 ** 40, H=2 ** 40), dict(NC=2 ** 50, W=2 ** 10, H=2 ** 10)):
    assert pool(**kw) == ENOTSUP and b'overflow' in err(), kw
  assert pool(NC=0) == 0 and pool(NC=0, src=None, out=None) == 0
  for name in ('spx_stencil_plan', 'spx_stencil', 'spx_maxpool'):
    assert name in backend.EXPORTED

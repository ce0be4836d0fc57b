"""Host-side logic of the expression engine (tiling, fusion, partial combine,
tile merge) on CPU, with the TEST-DOUBLE backend standing in for libspx.so.
Numerics of the real kernels are covered by the -m gpu tests."""
import numpy as np
import pytest

from oracle import rng
from oracle import spartan_cpu as O


@pytest.mark.parametrize('W', [1, 2, 3, 5, 8])
def test_reductions_all_workers(host_ctx, W):
  host_ctx(W)
  from spartan_amd import expr
  for shape in [(50,), (50, 50), (12, 7, 5)]:
    nx = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    x = expr.arange(shape, dtype=np.int64)
    for axis in [None] + list(range(len(shape))):
      np.testing.assert_array_equal(x.sum(axis).glom(), O.sum_tiles(nx, axis, W))
      np.testing.assert_array_equal(x.argmin(axis).glom(), O.arg_tiles(nx, axis, W))
      np.testing.assert_array_equal(x.argmax(axis).glom(), O.arg_tiles(nx, axis, W, 'argmax'))
      np.testing.assert_array_equal(expr.max(x, axis).glom(), O.max_tiles(nx, axis, W))


def test_fusion_builds_one_node(host_ctx):
  host_ctx(1)
  from spartan_amd import expr
  from spartan_amd.expr.map import MapExpr
  from spartan_amd.expr.reduce import ReduceExpr
  x = expr.rand(8, 8, dtype=np.float32, seed=1).force()
  y = expr.rand(8, 8, dtype=np.float32, seed=2).force()
  X, Y = expr.lazify(x), expr.lazify(y)
  e = expr.sum(X * Y + expr.exp(Y), axis=0).optimized()
  assert isinstance(e, ReduceExpr)
  assert len(e.children) == 3 or len(e.children) == 2
  assert not any(isinstance(c, MapExpr) for c in e.children)
  assert 'exp' in repr(e.op.deps[1])
  m = (X * Y + 1.0).optimized()
  assert isinstance(m, MapExpr) and not any(isinstance(c, MapExpr) for c in m.children)


def test_force_does_not_optimize_and_cache(host_ctx):
  host_ctx(1)
  from spartan_amd import expr
  a = expr.ones((4, 4))
  b = a + a
  r1 = b.force()
  r2 = b.force()
  assert r1 is r2  # expression cache (base.py:259-300)
  o = b.optimized()
  assert o is b.optimized()


def test_update_merge_semantics(host_ctx):
  host_ctx(3)
  import torch
  from spartan_amd.array import distarray, extent
  a = distarray.create((6, 4), np.float64, reducer=np.add)
  a.update(extent.create((0, 0), (6, 4), (6, 4)), np.ones((6, 4)))
  a.update(extent.create((1, 0), (3, 4), (6, 4)), np.full((2, 4), 5.0))
  want = np.ones((6, 4))
  want[1:3] += 5
  np.testing.assert_array_equal(a.glom(), want)
  b = distarray.create((6,), np.float64, reducer=np.maximum)
  b.update(extent.create((0,), (4,), (6,)), np.array([1., 9., 3., 4.]))
  b.update(extent.create((2,), (6,), (6,)), np.array([7., 2., 8., 8.]))
  np.testing.assert_array_equal(b.glom(), O_merge_expect())


def O_merge_expect():
  out = O.OArray((6,), np.float64, 3, reducer=np.maximum)
  out.update(O.ext_create((0,), (4,), (6,)), np.array([1., 9., 3., 4.]))
  out.update(O.ext_create((2,), (6,), (6,)), np.array([7., 2., 8., 8.]))
  return out.glom()


def test_dtype_rules(host_ctx):
  host_ctx(2)
  from spartan_amd import expr
  f = expr.ones((3,), dtype=np.float32)
  assert (f * 2.0).glom().dtype == np.float32        # weak python scalar
  assert (f + f).glom().dtype == np.float32
  i = expr.arange((4,), dtype=np.int32)
  assert (i + 1).glom().dtype == np.int32
  assert (i / 2).glom().dtype == np.float64
  assert expr.sum(i).glom().dtype == np.int32        # dtype_fn(input)
  assert expr.argmin(f).glom().dtype == np.int64
  np.testing.assert_array_equal(expr.mean(i).glom(), np.arange(4).sum() // 4)


def test_rand_is_tiling_independent(host_ctx):
  outs = []
  for W in (1, 3, 7):
    host_ctx(W)
    from spartan_amd import expr
    outs.append(expr.rand(13, 11, dtype=np.float32, seed=5).glom())
  for o in outs[1:]:
    np.testing.assert_array_equal(o, outs[0])
  np.testing.assert_array_equal(outs[0], rng.rand((13, 11), 5, np.float32))


def test_unlowerable_mapper_runs_like_the_reference(host_ctx):
  """A mapper the tracer cannot lower runs per tile in NumPy: np.sort works;
  a Python branch on an array's truth value fails exactly as it would in the
  reference's FnCallExpr.evaluate (NumPy's ValueError)."""
  host_ctx(1)
  import warnings
  from spartan_amd import expr
  x = expr.ones((4,))
  with warnings.catch_warnings():
    warnings.simplefilter('ignore', RuntimeWarning)
    np.testing.assert_array_equal(expr.map(x, lambda v: np.sort(v)).glom(), np.ones(4))
    with pytest.raises(ValueError):
      expr.map(x, lambda v: v if v > 0 else -v).glom()


def test_dot_paths(host_ctx):
  for W in (1, 2, 3):
    host_ctx(W)
    from spartan_amd import expr
    a = rng.rand((40, 30), 1, np.float64)
    b = rng.rand((30, 20), 2, np.float64)
    got = expr.dot(expr.from_numpy(a), expr.from_numpy(b)).glom()
    np.testing.assert_allclose(got, a @ b, rtol=1e-12)
    got = expr.dot(expr.from_numpy(a), b).glom()
    np.testing.assert_allclose(got, a @ b, rtol=1e-12)
    v = rng.rand((30,), 3, np.float64)
    np.testing.assert_allclose(expr.dot(expr.from_numpy(a), expr.from_numpy(v)).glom(), a @ v, rtol=1e-12)


def test_lreg_update_matches_oracle(host_ctx):
  from oracle import workloads as OW
  for W in (1, 3):
    host_ctx(W)
    from spartan_amd import expr, workloads
    n, d = 200, 8
    X = rng.rand((n, d), 41, np.float32)
    Yv = rng.rand((n, 1), 42, np.float32)
    w = rng.rand((d, 1), 43, np.float32)
    x, y = expr.from_numpy(X), expr.from_numpy(Yv)
    got = workloads.linear_regression_update(x, y, w, 1e-3)
    want = OW.linear_regression_update(X, Yv, w, 1e-3, W)
    np.testing.assert_allclose(got, want, rtol=1e-5)


def test_kmeans_driver_host(host_ctx):
  from oracle import workloads as OW
  for W in (1, 3):
    host_ctx(W)
    from spartan_amd import expr, workloads
    pts = rng.rand((600, 8), 21, np.float32)
    c, labels = workloads.kmeans_fit(expr.from_numpy(pts), 5, 3)
    c2, l2 = OW.kmeans_fit(pts, 5, 3, W)
    np.testing.assert_allclose(c, c2, rtol=1e-6)
    np.testing.assert_array_equal(labels.glom(), l2)


def test_kmeans_driver_empty_cluster_host(host_ctx):
  """kmeans_fit launches iteration i + 1 with device-divided centres before it
  reads iteration i's counts; an empty cluster (here a centre far from every
  point in iteration 0, and reseeds that stay empty) makes it relaunch the
  iteration with the host rule's reseeded centres -- the results must be the
  sequential loop's (the oracle's), centres and labels."""
  from oracle import workloads as OW
  for W in (1, 2):
    host_ctx(W)
    from spartan_amd import expr, workloads
    pts = rng.rand((400, 6), 23, np.float32)
    c0 = np.vstack([pts[:3].astype(np.float64), np.full((1, 6), 50.0), pts[3:4].astype(np.float64)])
    info = {}
    c, labels = workloads.kmeans_fit(expr.from_numpy(pts), 5, 4, centers=c0, info=info)
    c2, l2 = OW.kmeans_fit(pts, 5, 4, W, centers=c0)
    np.testing.assert_allclose(c, c2, rtol=1e-6)
    np.testing.assert_array_equal(labels.glom(), l2)
    _, l3 = OW.kmeans_fit(pts, 5, 1, W, centers=info['assign_centers'])
    np.testing.assert_array_equal(labels.glom(), l3)


def test_dot_reduce_fusion_rewrites_lreg(host_ctx):
  """DotReduceFusion folds dot(x, w_host) into the axis-0 reduction of
  x * (dot(x, w) - y): one ReduceExpr, no DotExpr left, same gradient."""
  host_ctx(2)
  from spartan_amd import expr
  from spartan_amd.config import FLAGS
  from spartan_amd.expr.dot import DotExpr
  from spartan_amd.expr.reduce import ReduceExpr
  n, d = 300, 16
  X = rng.rand((n, d), 41, np.float32)
  Yv = rng.rand((n, 1), 42, np.float32)
  w = rng.rand((d, 1), 43, np.float32)
  x, y = expr.from_numpy(X), expr.from_numpy(Yv)
  g = expr.sum(x * (expr.dot(x, w) - y), axis=0)
  opt = g.optimized()
  assert isinstance(opt, ReduceExpr)
  assert not any(isinstance(c, DotExpr) for c in opt.children)
  assert 'rowdot' in opt.op.pretty_str()
  got = opt.glom()
  want = (X * (X.dot(w) - Yv)).sum(0)
  np.testing.assert_allclose(got, want, rtol=1e-5)
  # not applied: axis 1, a wide w, or the flag off
  for e in (expr.sum(x * (expr.dot(x, w) - y), axis=1),
            expr.sum(x * expr.dot(x, np.ones((d, 1), np.float64)), axis=0)):
    assert any(isinstance(c, DotExpr) for c in e.optimized().children)
  FLAGS.opt_dot_fusion = False
  try:
    e = expr.sum(x * (expr.dot(x, w) - y), axis=0).optimized()
    assert any(isinstance(c, DotExpr) for c in e.children)
  finally:
    FLAGS.opt_dot_fusion = True


def test_dot_reduce_fusion_device_w(host_ctx):
  """DotReduceFusion with w a device-resident (K, 1) array (sgd_train keeps w
  on the GPU): the dot is still folded into the axis-0 reduction, and the
  device-w SGD loop is bit-identical to the host form (the same fp32 update,
  linear_regression_update) -- it only drops the per-iteration host round
  trip."""
  host_ctx(3)
  from spartan_amd import expr, workloads
  from spartan_amd.expr.dot import DotExpr
  from spartan_amd.expr.reduce import ReduceExpr
  n, d = 300, 16
  X = rng.rand((n, d), 41, np.float32)
  Yv = rng.rand((n, 1), 42, np.float32)
  w = rng.rand((d, 1), 43, np.float32)
  x = expr.lazify(expr.from_numpy(X).force())
  y = expr.lazify(expr.from_numpy(Yv).force())
  W = expr.lazify(expr.from_numpy(w).force())
  opt = expr.sum(x * (expr.dot(x, W) - y), axis=0).optimized()
  assert isinstance(opt, ReduceExpr)
  assert not any(isinstance(c, DotExpr) for c in opt.children)
  assert 'rowdot' in opt.op.pretty_str()
  np.testing.assert_array_equal(opt.glom(), expr.sum(x * (expr.dot(x, w) - y), axis=0).optimized().glom())
  w_dev = workloads.sgd_train(x, y, w, 1e-3, 5)
  w_host = workloads.sgd_train(x, y, w, 1e-3, 5, device_w=False)
  assert w_dev.dtype == w_host.dtype and w_dev.shape == w_host.shape
  np.testing.assert_array_equal(w_dev, w_host)


def test_automatic_tiling(host_ctx):
  """AutomaticTiling (optimize.py:454-890): a new 2-d array reduced over axis
  0 is partitioned by columns (each worker reduces whole columns: no partial
  exchange), over axis 1 by rows; values are unchanged; the flag turns it
  off."""
  host_ctx(4)
  from spartan_amd import expr
  from spartan_amd.config import FLAGS
  from spartan_amd.expr.ndarray import NdArrayExpr
  n, m = 40, 36
  X = rng.rand((n, m), 5, np.float64)

  def hints(e):
    out = []

    def walk(x):
      if isinstance(x, NdArrayExpr):
        out.append(tuple(x.tile_hint) if x.tile_hint is not None else None)
      for k in getattr(x, '_members', ()):
        v = getattr(x, k, None)
        for c in (v.vals if hasattr(v, 'vals') else [v]):
          if hasattr(c, '_members'):
            walk(c)
    walk(e)
    return out

  e0 = expr.sum(expr.rand(n, m, seed=5), axis=0).optimized()
  assert hints(e0) == [(n, 9)]
  np.testing.assert_allclose(e0.glom(), X.sum(0), rtol=1e-12)
  e1 = expr.sum(expr.rand(n, m, seed=5), axis=1).optimized()
  assert hints(e1) == [(10, m)]
  np.testing.assert_allclose(e1.glom(), X.sum(1), rtol=1e-12)
  d = expr.dot(expr.rand(n, m, seed=5), expr.rand(m, 20, seed=6)).optimized()
  np.testing.assert_allclose(d.glom(), X @ rng.rand((m, 20), 6, np.float64), rtol=1e-12)
  FLAGS.opt_auto_tiling = False
  try:
    assert hints(expr.sum(expr.rand(n, m, seed=5), axis=0).optimized()) == [None]
  finally:
    FLAGS.opt_auto_tiling = True


def test_dot_forced_operands(host_ctx):
  """dot() of already-forced DistArrays keeps them as device operands (the
  reference's dot takes any non-ndarray operand as an array, dot.py:238-283)."""
  import numpy as np
  from spartan_amd import expr
  host_ctx(2)
  a, b = expr.arange((30, 20)).force(), expr.arange((20, 10)).force()
  na, nb = np.arange(600.).reshape(30, 20), np.arange(200.).reshape(20, 10)
  np.testing.assert_array_equal(expr.dot(a, b).glom(), na @ nb)
  np.testing.assert_array_equal(expr.dot(a, expr.arange((20,)).force()).glom(), na @ np.arange(20.))


def test_map_forced_operands(host_ctx):
  """map / ufunc builtins over forced DistArrays: one operand each (the
  reference's util.is_iterable looks for __iter__, which a DistArray lacks),
  dtype from the array, never a host materialisation."""
  import numpy as np
  from spartan_amd import expr
  host_ctx(2)
  a = expr.arange((12, 8)).force()
  na = np.arange(96.).reshape(12, 8)
  np.testing.assert_array_equal(expr.map(a, np.sqrt).glom(), np.sqrt(na))
  np.testing.assert_array_equal(expr.map((a, a), np.add).glom(), na + na)
  np.testing.assert_array_equal(expr.astype(a, np.float32).glom(), na.astype(np.float32))
  np.testing.assert_allclose(expr.std(a, 0).glom(), na.std(0), rtol=1e-12)


def test_expr_method_surface(host_ctx):
  """Methods the reference attaches to Expr (spartan/expr/__init__.py:47-53)
  and the newaxis marker (base.py:23-26)."""
  host_ctx(2)
  from spartan_amd import expr
  from spartan_amd.expr import join
  for name in ('outer', 'sum', 'mean', 'astype', 'argmin', 'argmax'):
    assert callable(getattr(expr.Expr, name)), name
  assert expr.Expr.outer is join.outer
  x = expr.arange((6, 4))
  assert x[expr.newaxis, :, 1:3].shape == (1, 6, 2)
  assert x[:, None].shape == (6, 1, 4)
  assert x[2, None].shape == (1, 4)


def test_plan_cache_replays_structures(host_ctx):
  """expr/plan_cache.py: the second optimisation of an identical structure
  is a replay (no passes) with the new host values substituted, and gives
  the same results as a fresh optimisation; a different structure or
  different flags misses."""
  host_ctx(3)
  from spartan_amd import expr, workloads
  from spartan_amd.config import FLAGS
  from spartan_amd.expr import plan_cache
  from oracle import rng
  from oracle import workloads as OW
  Xn = rng.rand((300, 16), 41, np.float32)
  Yn = rng.rand((300, 1), 42, np.float32)
  w0 = rng.rand((16, 1), 43, np.float32)
  X, Y = expr.lazify(expr.from_numpy(Xn).force()), expr.lazify(expr.from_numpy(Yn).force())
  plan_cache.clear()
  h0 = plan_cache.STATS['hits']
  w_cached = workloads.sgd_train(X, Y, w0, 1e-3, 6)
  # iteration 1 misses; iteration 2 misses too, because iteration 1's
  # AutomaticTiling pinned a tiling on the X / Y nodes (part of the key, as a
  # fresh optimisation would read it); iterations 3-6 replay
  assert plan_cache.STATS['hits'] - h0 >= 4
  FLAGS.opt_plan_cache = False
  try:
    w_plain = workloads.sgd_train(X, Y, w0, 1e-3, 6)
  finally:
    FLAGS.opt_plan_cache = True
  np.testing.assert_array_equal(w_cached, w_plain)
  w = w0
  for _ in range(6):
    w = OW.linear_regression_update(Xn, Yn, w, 1e-3, 3)
  np.testing.assert_allclose(w_cached, w, rtol=1e-5)
  # same structure over other arrays / values: results follow the new leaves
  Zn = rng.rand((300, 16), 44, np.float32)
  Z = expr.lazify(expr.from_numpy(Zn).force())
  for a, an in ((X, Xn), (Z, Zn), (X, Xn)):
    for v in (w0, w0 * 2):
      got = expr.sum(a * (expr.dot(a, v) - Y), axis=0).optimized().glom()
      want = (an * (an @ v - Yn)).sum(0)
      np.testing.assert_allclose(got, want, rtol=1e-5)
  # a different reduction axis is a different structure
  m0 = plan_cache.STATS['misses']
  expr.sum(X * 2.0, axis=1).optimized().glom()
  expr.sum(X * 2.0, axis=0).optimized().glom()
  assert plan_cache.STATS['misses'] == m0 + 2
  np.testing.assert_allclose(expr.sum(X * 3.0, axis=0).optimized().glom(), (Xn * 3.0).sum(0), rtol=1e-5)


def test_plan_cache_keeps_shared_node_ids(host_ctx):
  """The reference's KMeans loop forces ``labels`` through ``counts`` and
  reuses the cached value for the centres (k_means_.py:129-136): with the
  plan cache replaying later iterations, the assignment still runs once per
  iteration (replayed nodes keep the ids of the nodes they stand for)."""
  host_ctx(1)
  from spartan_amd import backend, expr
  from spartan_amd.examples.kmeans import KMeans
  from spartan_amd.expr import plan_cache
  from oracle import rng
  pts = rng.rand((400, 8), 21, np.float32)
  X = expr.from_numpy(pts).force()
  be = backend.get()
  calls = []
  orig = be.kmeans_assign  # fp32 points: argmin(outer) fused with fp32-rounded distances
  be.kmeans_assign = lambda *a, **k: (calls.append(k.get('dist_dtype')), orig(*a, **k))[1]
  try:
    plan_cache.clear()
    h0 = plan_cache.STATS['hits']
    KMeans(5, 4).fit(X, pts[:5].astype(np.float64))
  finally:
    be.kmeans_assign = orig
  assert plan_cache.STATS['hits'] > h0
  assert calls == [np.float32] * 4


def test_kmeans_api_one_pass(host_ctx):
  """The drop-in KMeans loop in spx_kmeans_step's domain (fp32, D = 64,
  K <= 256): the fused argmin runs the step, and the centre / count joins of
  that labels array take its sums and counts instead of reading X again --
  same centres and labels as the two-pass joins."""
  host_ctx(1)
  from spartan_amd import backend, expr
  from spartan_amd.examples import kmeans as km
  from oracle import rng
  pts = rng.rand((600, 64), 23, np.float32)
  X = expr.from_numpy(pts).force()
  c0 = pts[:6].astype(np.float64)
  be = backend.get()
  calls = {'kmeans_step': 0, 'kmeans_accumulate': 0, 'bincount': 0, 'kmeans_assign': 0}
  origs = {n: getattr(be, n) for n in calls}

  def counted(n):
    def f(*a, **k):
      calls[n] += 1
      return origs[n](*a, **k)
    return f
  for n in calls:
    setattr(be, n, counted(n))
  try:
    c1, l1 = km.KMeans(6, 3).fit(X, c0)
    fused = dict(calls)
    for n in calls:
      calls[n] = 0
    dom = km._step_domain
    km._step_domain = lambda X, K: False
    try:
      c2, l2 = km.KMeans(6, 3).fit(X, c0)
    finally:
      km._step_domain = dom
  finally:
    for n, f in origs.items():
      setattr(be, n, f)
  assert fused['kmeans_step'] == 3 and fused['kmeans_accumulate'] == 3 and fused['bincount'] == 0
  assert calls['kmeans_step'] == 0 and calls['kmeans_assign'] == 3 and calls['bincount'] == 3
  np.testing.assert_array_equal(c1, c2)
  np.testing.assert_array_equal(l1.glom(), l2.glom())


def _km_case(expr):
  """(points, forced X, first centres) in spx_kmeans_step's domain."""
  pts = rng.rand((600, 64), 23, np.float32)
  return pts, expr.from_numpy(pts).force(), pts[:6].astype(np.float64)


def _km_handoff_empty(p):
  """No fused-step sums / counts, reduced counts, staged copies or queued step."""
  return all(v is None for v in (p.step_X, p.step_labels, p.step_sums, p.step_counts, p.red_counts,
                                 p.early_sums, p.early_counts, p.queued))


def test_kmeans_api_nothing_outlives_the_fit(host_ctx):
  """KMeans.fit leaves the joins' hand-off empty, and once the caller drops X
  and the labels (and the eval / plan caches) both are freed: the state the
  joins share refers to them weakly only."""
  host_ctx(1)
  import gc
  import weakref
  from spartan_amd import expr
  from spartan_amd.examples import kmeans as km
  from spartan_amd.expr import plan_cache
  from spartan_amd.expr.base import eval_cache
  pts, X, c0 = _km_case(expr)
  c, labels = km.KMeans(6, 3).fit(X, c0)
  assert _km_handoff_empty(km._PIPE) and not km._PIPE.following
  lab_arr = labels.force()
  assert lab_arr is labels.force()  # the array the joins were handed, not a new evaluation
  wx, wl = weakref.ref(X), weakref.ref(lab_arr)
  del X, labels, lab_arr
  eval_cache.clear()
  plan_cache.clear()
  gc.collect()
  assert wx() is None and wl() is None


def test_kmeans_api_failed_fit_leaves_nothing(host_ctx):
  """A fit that raises between the fused assignment and the joins leaves no
  hand-off behind and the 'another iteration follows' flag down; the next
  fit on the same X is bit-identical to one made before the failure."""
  host_ctx(1)
  from spartan_amd import backend, expr
  from spartan_amd.examples import kmeans as km
  pts, X, c0 = _km_case(expr)
  c1, l1 = km.KMeans(6, 3).fit(X, c0)
  l1 = l1.glom()
  be = backend.get()
  orig = be.kmeans_step
  n = [0]

  def failing(*a, **k):
    n[0] += 1
    if n[0] == 2:
      raise RuntimeError('kmeans_step: injected failure')
    return orig(*a, **k)
  be.kmeans_step = failing
  try:
    with pytest.raises(RuntimeError, match='injected'):
      km.KMeans(6, 3).fit(X, c0)
  finally:
    be.kmeans_step = orig
  assert n[0] == 2
  assert not km._PIPE.following and _km_handoff_empty(km._PIPE)
  c2, l2 = km.KMeans(6, 3).fit(X, c0)
  assert np.array_equal(c1.view(np.int64), c2.view(np.int64))
  np.testing.assert_array_equal(l1, l2.glom())


def test_kmeans_api_hand_written_loop_is_one_pass(host_ctx):
  """outer / argmin / the two map2s written by hand, without KMeans.fit: the
  count and centre joins still take the fused step's counts and sums (one
  pass over X), and they equal the two-pass joins'."""
  host_ctx(1)
  from spartan_amd import backend, expr
  from spartan_amd.examples import kmeans as km
  pts, X, c0 = _km_case(expr)
  be = backend.get()
  calls = {'kmeans_step': 0, 'kmeans_accumulate': 0, 'bincount': 0}
  origs = {n: getattr(be, n) for n in calls}

  def counted(n):
    def f(*a, **k):
      calls[n] += 1
      return origs[n](*a, **k)
    return f

  def one_iteration():
    labels = expr.argmin(expr.outer((X, expr.from_numpy(c0)), (0, 0), fn=km.kmeans_dist_mapper, shape=(600, 6)),
                         axis=1)
    lab = labels.optimized().glom()
    counts = expr.map2(labels, 0, fn=km.kmeans_count_mapper, fn_kw={'centers_count': 6}, shape=(6,))
    sums = expr.map2((X, labels), (0, 0), fn=km.kmeans_center_mapper, fn_kw={'centers_count': 6}, shape=(6, 64))
    return lab, counts.optimized().glom(), sums.optimized().glom()
  for n in calls:
    setattr(be, n, counted(n))
  try:
    l1, n1, s1 = one_iteration()
    fused = dict(calls)
    dom = km._step_domain
    km._step_domain = lambda X, K: False
    try:
      l2, n2, s2 = one_iteration()
    finally:
      km._step_domain = dom
  finally:
    for n, f in origs.items():
      setattr(be, n, f)
  # (the test double's kmeans_step makes one kmeans_accumulate call itself)
  assert fused == {'kmeans_step': 1, 'kmeans_accumulate': 1, 'bincount': 0}
  assert calls['kmeans_step'] == 1 and calls['bincount'] == 1 and calls['kmeans_accumulate'] == 2
  np.testing.assert_array_equal(l1, l2)
  np.testing.assert_array_equal(n1, n2)
  assert np.array_equal(s1.view(np.int32), s2.view(np.int32)) and n1.sum() == 600


def test_kmeans_row_cache_is_by_tile_identity(host_ctx):
  """_row_blocks keeps X's row blocks while every local tile tensor is the
  same object; a replaced tile tensor is gathered again."""
  host_ctx(1)
  from spartan_amd import expr
  from spartan_amd.examples import kmeans as km
  pts, X, c0 = _km_case(expr)
  blocks, got = km._row_blocks(X, 64)
  again = km._row_blocks(X, 64)
  assert again[0] is blocks and again[1] is got
  tile = next(iter(X.local.values()))
  old = tile.data
  tile.data = old.clone()
  blocks2, got2 = km._row_blocks(X, 64)
  assert blocks2 is not blocks and got2 is not got
  now = {t.data.untyped_storage().data_ptr() for t in X.local.values()}
  assert old.untyped_storage().data_ptr() not in now
  assert all(r.untyped_storage().data_ptr() in now for r in got2.values())
  np.testing.assert_array_equal(np.concatenate([got2[i].numpy() for i in sorted(got2)]), pts)
  assert km._row_blocks(X, 64)[0] is blocks2


def _host_mapper_cases(expr):
  """(name, expression, NumPy result) for mappers that cannot be traced into
  a kernel -- data-dependent control flow, non-ufunc NumPy calls on the tile
  -- which the reference simply runs per tile (local.py:110-122)."""
  a = np.arange(60.0).reshape(6, 10)[:, ::-1] % 7.0
  x = expr.from_numpy(a)

  def branchy(t):
    if t.sum() > 100:       # a Python branch on the tile's data
      return t * 2.0
    return t - 1.0

  def want_branchy(strips):
    return np.concatenate([branchy(s) for s in strips])

  return a, x, branchy, want_branchy


@pytest.mark.parametrize('W', [1, 3])
def test_untraceable_mapper_runs_on_host(host_ctx, W):
  host_ctx(W)
  from spartan_amd import expr
  from spartan_amd.expr import engine
  from spartan_amd.array import distarray
  a, x, branchy, _ = _host_mapper_cases(expr)
  n0 = engine.HOST_MAPPER_CALLS[0]
  with pytest.warns(RuntimeWarning, match='host'):
    got = expr.map(x, lambda t: np.sort(t, axis=1)).glom()
  np.testing.assert_array_equal(got, np.sort(a, axis=1))
  assert engine.HOST_MAPPER_CALLS[0] - n0 == len(distarray.from_numpy(a).tiles)
  # a branch on the tile's values: per tile, as the reference evaluates it
  strips = [a[ex.ul[0]:ex.lr[0]] for ex in sorted(distarray.from_numpy(a).tiles, key=lambda e: e.ul)]
  got = expr.map(x, branchy).glom()
  np.testing.assert_array_equal(got, np.concatenate([branchy(s) for s in strips]))
  # the same mapper inside a reduction: host map, device reduction
  np.testing.assert_array_equal(expr.sum(expr.map(x, branchy), axis=0).optimized().glom(),
                                np.concatenate([branchy(s) for s in strips]).sum(0))
  # ufunc trees never take the host path
  n1 = engine.HOST_MAPPER_CALLS[0]
  np.testing.assert_array_equal((x * 2.0 + 1.0).glom(), a * 2.0 + 1.0)
  np.testing.assert_array_equal(expr.map(x, lambda t: t * t).glom(), a * a)
  assert engine.HOST_MAPPER_CALLS[0] == n1
  # the reference's shape assertion (map.py:80-82)
  with pytest.raises(AssertionError):
    expr.map(x, lambda t: np.sort(t, axis=None)[:3]).glom()


def test_replayed_plans_keep_the_sign_of_zero(host_ctx):
  """A 0-d host scalar is a plan-cache slot; the lowering memo of a replayed
  tree must not hand -0.0 the lowering made for +0.0 (the sign survives a
  division: +inf / -inf)."""
  host_ctx(1)
  from spartan_amd import expr
  X = expr.lazify(expr.from_numpy(np.ones((4, 3))).force())
  for _ in range(2):
    for s, inf in ((np.array(0.0), np.inf), (np.array(-0.0), -np.inf)):
      with np.errstate(divide='ignore'):
        got = (1.0 / (X * s)).optimized().glom()
      np.testing.assert_array_equal(got, np.full((4, 3), inf))


def test_tiny_uploads_of_other_dtypes(host_ctx):
  """Small host arrays of dtypes outside the backend's five (float16,
  int8, big-endian) take the plain upload path instead of failing."""
  host_ctx(1)
  import torch
  from spartan_amd.array import transfer
  for a in (np.arange(6, dtype=np.float16), np.arange(6, dtype=np.int8), np.arange(6, dtype='>f8')):
    t = transfer.upload(a, torch.device('cpu'))
    np.testing.assert_array_equal(t.numpy().astype(np.float64), a.astype(np.float64))


class _Ev:
  """Stand-in for a torch.cuda.Event (host logic only): counts its waits."""
  n = 0

  def synchronize(self):
    _Ev.n += 1


def test_download_host_shadow_is_one_shot_and_versioned():
  """array/transfer.py host shadows (examples/kmeans.py speculation): the next
  download of the tensor reads the attached host copy after waiting for its
  event; the entry is taken once; an in-place change of the tensor since
  the attach (torch version counter) or another tensor ignores it."""
  import torch
  from spartan_amd.array import transfer
  t = torch.arange(6, dtype=torch.float64).reshape(2, 3)
  host = np.full((2, 3), 7.0)
  n0 = _Ev.n
  transfer.attach_shadow(t, host, _Ev())
  np.testing.assert_array_equal(transfer.download(t), host)
  assert _Ev.n == n0 + 1
  np.testing.assert_array_equal(transfer.download(t), t.numpy())   # one-shot
  transfer.attach_shadow(t, host, _Ev())
  t.add_(1.0)                                                       # written since: stale
  np.testing.assert_array_equal(transfer.download(t), t.numpy())
  u = torch.zeros((2, 3), dtype=torch.float64)
  transfer.attach_shadow(t, host, _Ev())
  np.testing.assert_array_equal(transfer.download(u), u.numpy())   # another tensor
  transfer._SHADOWS.clear()


def test_upload_alias_bitwise_and_one_shot():
  """array/transfer.py upload aliases: the registered tensor is handed out
  only for an array bit-identical to its host copy (-0.0 vs 0.0 differ),
  of the same shape and dtype; one-shot either way."""
  import torch
  from spartan_amd.array import transfer
  dev = torch.tensor([[1.0, -0.0], [2.5, 3.0]], dtype=torch.float64)
  host = dev.numpy().copy()
  cpu = torch.device('cpu')
  transfer.register_upload_alias(host, dev, _Ev())
  assert transfer._take_alias(host.copy(), cpu) is dev
  assert not transfer._ALIAS
  transfer.register_upload_alias(host, dev, _Ev())
  other = host.copy()
  other[0, 1] = 0.0                                                 # +0.0: not bit-identical
  assert transfer._take_alias(other, cpu) is None
  assert not transfer._ALIAS
  transfer.register_upload_alias(host, dev, _Ev())
  assert transfer._take_alias(host.reshape(4), cpu) is None         # shape differs
  transfer.register_upload_alias(host, dev, _Ev())
  assert transfer._take_alias(host.astype(np.float32), cpu) is None  # dtype differs


def test_shadow_and_alias_withdrawal():
  """array/transfer.py drop_shadow / drop_upload_alias: a producer about to
  reuse its host copy withdraws the entry; a withdrawn shadow is not served by
  download nor a withdrawn alias by upload; dropping for another tensor
  leaves the entry in place."""
  import torch
  from spartan_amd.array import transfer
  t = torch.arange(6, dtype=torch.float64).reshape(2, 3)
  u = torch.zeros((2, 3), dtype=torch.float64)
  host = np.full((2, 3), 7.0)
  n0 = _Ev.n
  transfer.attach_shadow(t, host, _Ev())
  transfer.drop_shadow(u)                                           # another tensor: stays
  np.testing.assert_array_equal(transfer.download(t), host)
  assert _Ev.n == n0 + 1
  transfer.attach_shadow(t, host, _Ev())
  transfer.drop_shadow(t)
  assert not transfer._SHADOWS
  np.testing.assert_array_equal(transfer.download(t), t.numpy())   # not served
  assert _Ev.n == n0 + 1
  cpu = torch.device('cpu')
  transfer.register_upload_alias(t.numpy().copy(), t, _Ev())
  transfer.drop_upload_alias(u)                                     # another tensor: stays
  assert transfer._take_alias(t.numpy().copy(), cpu) is t
  transfer.register_upload_alias(t.numpy().copy(), t, _Ev())
  transfer.drop_upload_alias(t)
  assert not transfer._ALIAS
  up = transfer.upload(t.numpy().copy(), cpu)
  assert up is not t and _Ev.n == n0 + 2
  np.testing.assert_array_equal(up.numpy(), t.numpy())

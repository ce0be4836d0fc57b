"""``spartan_amd.fuzzy_assign`` / ``fuzzy_membership`` and
``examples.fuzzy_kmeans`` host logic (no GPU): the yardstick's own identities,
the pinned divergence from the reference, every layout of the expression layer
over worker counts, laziness, validation, the driver against a NumPy loop, and
the argument checks and plan answers of spx_fuzzy_step / spx_fuzzy_plan.

The expression layer runs here over the CPU test double whose ``fuzzy_step`` is
the yardstick (fuzzy_ref.FuzzyFakeBackend); the kernel itself is tested on the
GPU in tests/test_fuzzy_gpu.py.
"""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, 'spartan_amd', 'libspx.so')

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')

N, D, K = 10, 6, 3
HINTS = [(N, D), (4, D), (N, 3), (4, 3)]


@pytest.fixture
def fuzzy_ctx(host_ctx):
  """host_ctx with the fuzzy-capable test double installed."""
  from spartan_amd import backend
  from fuzzy_ref import FuzzyFakeBackend

  def make(num_workers=1):
    host_ctx(num_workers)
    be = FuzzyFakeBackend()
    backend.set_backend(be)
    return be
  return make


def _data(dtype=np.float64, seed=5):
  r = np.random.RandomState(seed)
  return r.randn(N, D).astype(dtype), r.randn(K, D)


# --------------------------------------------------------------- yardstick
def test_yardstick_identities():
  """The K^2 form and the O(K) form agree within 1e-14 on every GPU shape;
  rows of U sum to 1; the label is the nearest centre and the largest
  membership."""
  from fuzzy_ref import SHAPES, fuzzy_data, fuzzy_ref, membership_ok
  for (n, d, k, m) in SHAPES:
    X, C = fuzzy_data(n, d, k, np.float64)
    r = fuzzy_ref(X, C, 2.0 / (m - 1.0))
    assert np.abs(r['U'] - membership_ok(r['dist'], 2.0 / (m - 1.0))).max() <= 1e-14
    np.testing.assert_allclose(r['U'].sum(axis=1), 1.0, rtol=0, atol=1e-13)
    assert np.array_equal(r['labels'], np.argmin(r['dist'], axis=1))
    assert np.array_equal(r['labels'], np.argmax(r['U'], axis=1))
    np.testing.assert_allclose(r['counts'].sum(), n, rtol=1e-13)
    if n > 3:  # the planted row: membership 1 in centre 0, where a plain d^-e overflows at m = 1.1
      assert r['labels'][3] == 0 and r['U'][3, 0] > 1 - 1e-9


def test_reference_live_expression_picks_the_farthest_centre():
  """The divergence pin.  The reference's live code divides
  reshape(d, (n, 1, k)) by reshape(d, (n, k, 1)) and sums over axis 2: the
  membership grows with the distance, so argmax names the FARTHEST centre on
  every row.  The rule built here names the nearest."""
  from fuzzy_ref import fuzzy_ref
  r = np.random.RandomState(0)
  X, C = r.randn(50, 4), r.randn(5, 4)
  d = ((X[:, None, :] - C[None, :, :]) ** 2).sum(axis=2) + 1e-11
  prob = 1.0 / ((d[:, None, :] / d[:, :, None]) ** 2.0).sum(axis=2)
  assert np.array_equal(np.argmax(prob, axis=1), np.argmax(d, axis=1))
  assert not np.array_equal(np.argmax(prob, axis=1), np.argmin(d, axis=1))
  assert np.array_equal(fuzzy_ref(X, C, 2.0)['labels'], np.argmin(d, axis=1))


# ------------------------------------------------------------- expr layer
@pytest.mark.parametrize('W', [1, 2, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_fuzzy_every_layout(fuzzy_ctx, W, dtype):
  import torch
  be = fuzzy_ctx(W)
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from fuzzy_ref import fuzzy_ref
  X, C = _data(dtype)
  want = fuzzy_ref(X, C, 2.0 / (1.7 - 1.0), 1e-11, 1.0)
  first = None
  for hint in HINTS + ['replicated', 'host']:
    if hint == 'replicated':
      x = expr.lazify(distarray.ReplicatedArray(torch.as_tensor(X.copy())))
    elif hint == 'host':
      x = X
    else:
      x = expr.lazify(expr.from_numpy(X, tile_hint=hint).force())
    del be.calls[:]
    labels, counts, sums = expr.fuzzy_assign(x, C, m=1.7)
    assert labels.shape == (N,) and labels.dtype == np.int64
    assert counts.shape == (K,) and counts.dtype == np.float64
    assert sums.shape == (K, D) and sums.dtype == np.float64
    assert 'fuzzy_step' not in be.calls  # lazy
    got_counts = counts.glom()
    if isinstance(hint, tuple):
      cuts = sorted({(e.ul[0], e.lr[0]) for e in x.val.tiles})
      assert be.calls.count('fuzzy_step') == len(cuts), hint  # one launch per row slab
      lab = labels.force()
      assert sorted((e.ul[0], e.lr[0]) for e in lab.tiles) == cuts, hint  # tiled at X's row cuts
    elif hint == 'replicated':
      assert be.calls.count('fuzzy_step') == 1
      assert isinstance(labels.force(), distarray.ReplicatedArray)
    else:  # a host array is distributed by the default tiling first
      assert be.calls.count('fuzzy_step') >= 1
    steps = be.calls.count('fuzzy_step')
    got = (labels.glom(), got_counts, sums.glom())
    assert be.calls.count('fuzzy_step') == steps, hint  # the triple evaluated once
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want['labels']), hint
    np.testing.assert_allclose(got[1], want['counts'], rtol=1e-13, err_msg=str(hint))
    np.testing.assert_allclose(got[2], want['sums'], rtol=1e-12, atol=1e-13, err_msg=str(hint))
    if isinstance(hint, tuple) and hint[0] == 4:  # the slabs' sums add up in one order for both column layouts
      if first is None:
        first = got
      else:
        assert all(np.array_equal(a, b) for a, b in zip(first, got))

    del be.calls[:]
    U = expr.fuzzy_membership(x, C, m=1.7)
    assert U.shape == (N, K) and U.dtype == np.dtype(dtype) and 'fuzzy_step' not in be.calls
    u = U.force()
    if isinstance(hint, tuple):
      assert sorted((e.ul[0], e.lr[0]) for e in u.tiles) == cuts and all(e.ul[1] == 0 and e.lr[1] == K for e in u.tiles)
    assert np.array_equal(u.glom(), want['U'].astype(dtype)), hint


def test_weight_power_reaches_the_step(fuzzy_ctx):
  fuzzy_ctx(2)
  from spartan_amd import expr
  from fuzzy_ref import fuzzy_ref
  X, C = _data()
  want = fuzzy_ref(X, C, 2.0, 1e-3, 2.0)
  _labels, counts, sums = expr.fuzzy_assign(expr.from_numpy(X, tile_hint=(4, 3)), C, m=2.0, eps=1e-3, weight_power=2.0)
  np.testing.assert_allclose(counts.glom(), want['counts'], rtol=1e-13)
  np.testing.assert_allclose(sums.glom(), want['sums'], rtol=1e-12, atol=1e-13)


def test_validation_errors(fuzzy_ctx):
  fuzzy_ctx(1)
  import scipy.sparse as sp
  from spartan_amd import expr
  X, C = _data()
  for fn in (expr.fuzzy_assign, expr.fuzzy_membership):
    for bad in (1.0, 0.5, float('nan'), float('inf')):
      with pytest.raises(ValueError, match='fuzzifier m'):
        fn(X, C, m=bad)
    for bad in (0.0, -1e-3, float('nan')):
      with pytest.raises(ValueError, match='eps'):
        fn(X, C, eps=bad)
    for bad in (np.ones(4), np.ones((2, 3, 6))):
      with pytest.raises(ValueError, match='2-d array of points'):
        fn(bad, C)
    for bad in (np.ones((3, 5)), np.ones(6), np.ones((0, 6))):
      with pytest.raises(ValueError, match='centre'):
        fn(X, bad)
    with pytest.raises(TypeError, match='float32 / float64'):
      fn(X.astype(np.int64), C)
    with pytest.raises(TypeError, match=r'todense\(\)'):
      fn(sp.csr_matrix(X), C)
    with pytest.raises(TypeError, match=r'todense\(\)'):
      fn(X, sp.csr_matrix(C))
  for bad in (0.0, -1.0, float('nan')):
    with pytest.raises(ValueError, match='weight_power'):
      expr.fuzzy_assign(X, C, weight_power=bad)


# ------------------------------------------------------------------ driver
@pytest.mark.parametrize('weight_power', [1.0, 2.0])
def test_driver_against_numpy_loop(fuzzy_ctx, weight_power):
  be = fuzzy_ctx(2)
  from spartan_amd import expr
  from spartan_amd.examples.fuzzy_kmeans import fuzzy_kmeans
  r = np.random.RandomState(11)
  X = np.concatenate([r.randn(20, 4) + 4 * c for c in range(3)])
  C0 = X[[0, 25, 45]].copy() + 0.1
  # the NumPy loop
  C, e = C0.copy(), 2.0 / (1.8 - 1.0)
  for _ in range(3):
    d = ((X[:, None, :] - C[None, :, :]) ** 2).sum(axis=2) + 1e-11
    U = 1.0 / ((d[:, :, None] / d[:, None, :]) ** e).sum(axis=2)
    Wt = U ** weight_power
    want_labels = np.argmin(d, axis=1)
    C = (Wt.T @ X) / Wt.sum(axis=0)[:, None]
  labels, centers = fuzzy_kmeans(expr.from_numpy(X, tile_hint=(16, 4)), k=3, num_iter=3, m=1.8, centers=C0,
                                 weight_power=weight_power, return_centers=True)
  assert be.calls.count('fuzzy_step') == 3 * 4  # four row slabs an iteration
  assert np.array_equal(labels.glom(), want_labels)
  assert centers.dtype == np.float64 and np.abs(centers - C).max() <= 1e-12
  only = fuzzy_kmeans(X, k=3, num_iter=1, m=1.8, centers=C0)
  assert isinstance(only, expr.Expr) and only.shape == (60,)


def test_driver_reseeds_an_empty_centre(fuzzy_ctx):
  be = fuzzy_ctx(1)
  from spartan_amd.examples.fuzzy_kmeans import fuzzy_kmeans
  from fuzzy_ref import fuzzy_ref
  X, C0 = _data()
  be.zero_counts = (1,)
  _labels, centers = fuzzy_kmeans(X, k=K, num_iter=1, centers=C0, seed=3, return_centers=True)
  want = fuzzy_ref(X, C0, 2.0)
  new = want['sums'] / want['counts'][:, None]
  new[1] = np.random.default_rng(3).random((1, D))[0]  # the seeded generator's first draw, count 1
  assert np.all(np.isfinite(centers)) and np.abs(centers - new).max() <= 1e-12
  again = fuzzy_kmeans(X, k=K, num_iter=1, centers=C0, seed=3, return_centers=True)[1]
  assert np.array_equal(centers, again)
  with pytest.raises(ValueError, match='centres must be'):
    fuzzy_kmeans(X, k=K + 1, num_iter=1, centers=C0)


# ------------------------------------------------------ the C ABI, no GPU
def _lib():
  import torch  # noqa: F401  (torch's HIP runtime first)
  from spartan_amd import binding
  return binding.load_library(), binding


@needs_lib
def test_plan_answers_without_gpu():
  lib, binding = _lib()
  for dtype in (np.float32, np.float64):
    plans = [binding.fuzzy_plan(dtype, n, 128, 256) for n in (0, 1, 1000, 1 << 22)]
    rt, g, kmax, nbytes = plans[0]
    assert rt >= 1 and g >= 1 and kmax >= 256 and nbytes > 0
    assert all(p == plans[0] for p in plans)  # nothing depends on N
    assert binding.fuzzy_plan(dtype, 10, 128, 64)[3] < nbytes
    assert binding.fuzzy_plan(dtype, 10, 5, kmax + 1) == (rt, g, kmax, None)
  with pytest.raises(TypeError, match='float32 / float64'):
    binding.fuzzy_plan(np.int32, 1, 1, 1)
  with pytest.raises(ValueError, match='bad sizes'):
    binding.fuzzy_plan(np.float32, 1, 0, 1)


@needs_lib
def test_argument_checks_without_gpu():
  lib, binding = _lib()
  F32, I64, EINVAL, ENOTSUP = binding.SPX_F32, binding.SPX_I64, -1, -3
  kmax = binding.fuzzy_plan(np.float32, 1, 4, 1)[2]
  p = ctypes.c_void_p(4096)  # never dereferenced: every case fails its checks before any device work
  nul = ctypes.c_void_p(0)
  big = ctypes.c_size_t(1 << 40)

  def step(dtype=F32, N=5, D=4, K=3, points=p, ldp=4, centers=p, ex=2.0, eps=1e-11, wp=1.0, labels=nul, U=nul, ldu=3,
           sums=p, counts=p, ws=p, nws=big):
    return lib.spx_fuzzy_step(dtype, N, D, K, points, ldp, centers, ex, eps, wp, labels, U, ldu, sums, counts, 1, ws,
                              nws, nul)

  def err():
    return lib.spx_last_error().decode()

  assert step(dtype=I64) == ENOTSUP and 'float32 / float64' in err()
  assert step(dtype=9) == EINVAL and 'bad dtype' in err()
  assert step(K=0) == EINVAL and 'K >= 1' in err()
  assert step(K=kmax + 1) == ENOTSUP and 'kmax = %d' % kmax in err()
  for bad in (0.0, -2.0, float('nan'), float('inf')):
    assert step(ex=bad) == EINVAL and 'exponent' in err()
  for bad in (0.0, -1e-11, float('nan')):
    assert step(eps=bad) == EINVAL and 'eps' in err()
  for bad in (float('nan'), 0.0, float('inf')):
    assert step(wp=bad) == EINVAL and 'weight_power' in err()
  assert step(ldp=3) == EINVAL and 'ldp = 3 is below D = 4' in err()
  assert step(U=p, ldu=2) == EINVAL and 'ldu = 2 is below K = 3' in err()
  assert step(sums=nul) == EINVAL and 'null pointer' in err()
  assert step(counts=nul) == EINVAL and 'null pointer' in err()
  assert step(points=nul) == EINVAL and 'null pointer' in err()
  assert step(nws=ctypes.c_size_t(8)) == EINVAL and 'workspace' in err()
  assert step(N=-1) == EINVAL
  # N == 0 looks at no points pointer and launches nothing (zero_first off: sums / counts stay as they are)
  assert lib.spx_fuzzy_step(F32, 0, 4, 3, nul, 0, nul, 2.0, 1e-11, 1.0, nul, nul, 0, p, p, 0, nul, 0, nul) == 0


@needs_lib
def test_backend_wrapper_checks_without_gpu():
  """HipBackend.fuzzy_step refuses what the kernel does not serve before any call."""
  import torch
  from spartan_amd import backend
  be = backend.HipBackend.__new__(backend.HipBackend)
  be._fuzzy_ws = {}
  c = torch.zeros((3, 4), dtype=torch.float64)
  x = torch.zeros((5, 4), dtype=torch.float32)
  kmax = backend.fuzzy_plan(np.float32, 5, 4, 3)[2]
  with pytest.raises(ValueError, match='2-d'):
    be.fuzzy_step(x[0], c, 2.0, 1e-11, 1.0, True, False)
  with pytest.raises(ValueError, match='float32 / float64'):
    be.fuzzy_step(x.to(torch.int64), c, 2.0, 1e-11, 1.0, True, False)
  with pytest.raises(ValueError, match='unit stride'):
    be.fuzzy_step(torch.zeros((4, 5), dtype=torch.float32).t(), c, 2.0, 1e-11, 1.0, True, False)
  with pytest.raises(ValueError, match='centers'):
    be.fuzzy_step(x, c.to(torch.float32), 2.0, 1e-11, 1.0, True, False)
  with pytest.raises(ValueError, match='exponent'):
    be.fuzzy_step(x, c, 0.0, 1e-11, 1.0, True, False)
  with pytest.raises(NotImplementedError, match='kmax = %d' % kmax):
    be.fuzzy_step(x, torch.zeros((kmax + 1, 4), dtype=torch.float64), 2.0, 1e-11, 1.0, True, False)
  with pytest.raises(ValueError, match='together'):
    be.fuzzy_step(x, c, 2.0, 1e-11, 1.0, True, False, sums=torch.zeros((3, 4), dtype=torch.float64))

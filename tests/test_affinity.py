"""``pairwise_kernel`` / ``normalized_affinity`` and
``examples.spectral_clustering`` host logic (no GPU): the yardstick's own
identities and the bound it is used with, the pinned divergence from the
reference's ``scaled_euclidean_distance``, every layout of the expression layer
over worker counts, laziness and sharing, the refusals, the driver on separated
blobs and against a NumPy model of its chain, and the plan answers and argument
checks of spx_pairwise_plan / spx_pairwise.

The expression layer runs here over the CPU test double whose ``pairwise`` is
the yardstick (affinity_ref.AffinityFakeBackend); the kernel itself is tested
on the GPU in tests/test_affinity_gpu.py.
"""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, 'spartan_amd', 'libspx.so')

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')

N, M, DIM = 11, 7, 3


@pytest.fixture
def aff_ctx(host_ctx):
  """host_ctx with the pairwise-capable test double installed."""
  from spartan_amd import backend
  from affinity_ref import AffinityFakeBackend

  def make(num_workers=1):
    host_ctx(num_workers)
    be = AffinityFakeBackend()
    backend.set_backend(be)
    return be
  return make


# --------------------------------------------------------------- yardstick
def test_yardstick_identities():
  from affinity_ref import METRICS, affinity_ref, pairwise_ref, points
  X = np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 4.0]])
  Y = np.array([[0.0, 0.0], [6.0, 8.0]])
  assert np.array_equal(pairwise_ref(X, Y, 'sqeuclidean')[0], [[0.0, 100.0], [25.0, 25.0], [25.0, 25.0]])
  assert np.array_equal(pairwise_ref(X, Y, 'euclidean')[0], [[0.0, 10.0], [5.0, 5.0], [5.0, 5.0]])
  assert np.array_equal(pairwise_ref(X, Y, 'manhattan')[0], [[0.0, 14.0], [7.0, 7.0], [7.0, 7.0]])
  v, gs = pairwise_ref(X, Y, 'rbf', 0.01)
  assert np.array_equal(gs, [[0.0, 1.0], [0.25, 0.25], [0.25, 0.25]]) and np.array_equal(v, np.exp(-gs))
  # identical rows: exactly 0 (rbf: exactly 1); Y = X: symmetric, bit for bit
  P = points(40, 5, np.float64, 1)
  P[7] = P[3]
  for metric in METRICS:
    a, gs = pairwise_ref(P, None, metric, 0.1)
    assert np.array_equal(a, a.T) and np.array_equal(gs, gs.T), metric
    same = 1.0 if metric == 'rbf' else 0.0
    assert np.all(np.diag(a) == same) and a[3, 7] == same, metric
  # a huge gamma s is 0, not an error; a NaN coordinate poisons its row and column only
  assert pairwise_ref(X, Y, 'rbf', 1e300)[0][0, 1] == 0.0
  P[5, 2] = np.nan
  a = pairwise_ref(P, None, 'rbf', 0.1)[0]
  mask = np.zeros((40, 40), bool)
  mask[5, :] = mask[:, 5] = True
  assert np.array_equal(np.isnan(a), mask)
  # the normalised form: D the row sums, L = A / sqrt(D_i D_j), the diagonal as given, symmetric
  Q = points(30, 4, np.float64, 2)
  L, D, A, _gs = affinity_ref(Q, 'rbf', 0.2, 1.0)
  np.testing.assert_allclose(D, A.sum(axis=1), rtol=1e-15)
  np.testing.assert_allclose(L[2, 9], A[2, 9] / np.sqrt(D[2] * D[9]), rtol=1e-14)
  assert np.array_equal(L, L.T) and np.all(np.diag(L) == 1.0)
  assert np.all(np.diag(affinity_ref(Q, 'rbf', 0.2, 0.25)[0]) == 0.25)
  # a degree of 0 is scaled by 1: one point has D = 0 under a distance metric, and L stays finite
  L1, D1, _A, _gs = affinity_ref(np.ones((1, 3)), 'euclidean')
  assert D1[0] == 0.0 and L1[0, 0] == 1.0
  Z = np.zeros((3, 2))
  Lz, Dz, _A, _gs = affinity_ref(Z, 'sqeuclidean', diagonal=5.0)
  assert np.array_equal(Dz, np.zeros(3)) and np.array_equal(Lz, 5.0 * np.eye(3))


def test_float32_arithmetic_stays_inside_the_bound():
  """Before the bound judges a kernel: the same formula in plain float32 NumPy
  is inside it for every input of the GPU tests."""
  from affinity_ref import (METRICS, assert_degrees_within, assert_within, edge_shapes, float32_model, from_sums,
                            gamma_for, pair_sums, points)
  worst = 0.0
  for n, m, d in edge_shapes(64, 16):
    X, Y = points(n, d, np.float32, 3), points(m, d, np.float32, 4)
    Y[1] = X[2]  # a duplicate row
    s, l1 = pair_sums(X, Y)
    for metric in METRICS:
      ref, gs = from_sums(s, l1, metric, gamma_for(d))
      got = float32_model(X, Y, metric, gamma_for(d))
      worst = max(worst, assert_within(got, ref, gs, np.float32, (n, m, d, metric)))
      assert_degrees_within(got.astype(np.float64).sum(axis=1), ref, gs, np.float32, (n, m, d, metric))
      assert got[2, 1] == (1.0 if metric == 'rbf' else 0.0)
  assert 0.0 < worst < 0.5  # room to spare: the kernel's fused multiply-add rounds less, not more


def test_reference_scaled_euclidean_ignores_the_difference():
  """The divergence pin.  The reference's ``scaled_euclidean_distance`` calls
  ``np.square(X, Y)``: NumPy reads the second argument as ``out``, so the call
  squares X INTO Y and never forms X - Y.  The rule of its docstring --
  exp(-sum / (2 (1.5 median)^2)) over the squared DIFFERENCES of the features
  -- gives another number, and needs a median over the features of every
  pair.  The driver built here refuses the name."""
  def live(X, Y):  # the reference's function body, typed out
    diff = np.square(X, Y)
    median = np.median(diff)
    total = diff.sum()
    return 0 if median == 0 else np.exp((-total) / (((median * 1.5) ** 2) * 2))

  def documented(X, Y):
    diff = np.square(X - Y)
    median = np.median(diff)
    return 0 if median == 0 else np.exp((-diff.sum()) / (((median * 1.5) ** 2) * 2))

  X = np.array([1.0, 2.0, 3.0])
  Y = np.array([1.5, 1.0, 5.0])
  Y_live = Y.copy()
  got = live(X, Y_live)
  assert np.array_equal(Y_live, np.square(X))  # the second point was overwritten with X^2 ...
  assert got == live(X, np.array([-7.0, 0.0, 9.0])) == live(X, X.copy())  # ... and never entered the value
  want = documented(X, Y)
  assert not np.isclose(got, want, rtol=1e-3) and 0 < want < 1
  assert live(X, X.copy()) != 1.0 and documented(X, X) == 0  # not even a point with itself
  from spartan_amd import expr
  from spartan_amd.examples.spectral_clustering import spectral_cluster
  pts = np.random.RandomState(0).rand(6, 2)
  with pytest.raises(ValueError, match='scaled_euclidean.*not built'):
    spectral_cluster(pts, 2, 2, 'scaled_euclidean')
  with pytest.raises(ValueError, match='scaled_euclidean.*not built'):
    expr.pairwise_kernel(pts, metric='scaled_euclidean')
  with pytest.raises(ValueError, match='scaled_euclidean.*not built'):
    expr.normalized_affinity(pts, metric='scaled_euclidean')


# ------------------------------------------------------------- expr layer
def _operand(expr, distarray, torch, a, hint):
  if hint == 'replicated':
    return expr.lazify(distarray.ReplicatedArray(torch.as_tensor(a.copy())))
  if hint == 'host':
    return a
  return expr.lazify(expr.from_numpy(a, tile_hint=hint).force())


HINTS = [(N, DIM), (4, DIM), (3, DIM), (7, 2), 'replicated', 'host']


@pytest.mark.parametrize('W', [1, 2, 3, 4])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_pairwise_kernel_every_layout(aff_ctx, W, dtype):
  import torch
  be = aff_ctx(W)
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from affinity_ref import pairwise_ref, points
  X, Y = points(N, DIM, dtype, 1), points(M, DIM, dtype, 2)
  for metric, gamma in (('rbf', 0.3), ('manhattan', 1.0)):
    want_xy = pairwise_ref(X, Y, metric, gamma)[0].astype(dtype)
    want_xx = pairwise_ref(X, None, metric, gamma)[0].astype(dtype)
    for hint in HINTS:
      for partner in ('self', 'tiled', 'host'):
        x = _operand(expr, distarray, torch, X, hint)
        y = None if partner == 'self' else (Y if partner == 'host' else
                                            expr.lazify(expr.from_numpy(Y, tile_hint=(3, 2)).force()))
        del be.calls[:], be.pairwise_calls[:]
        node = expr.pairwise_kernel(x, y, metric=metric, gamma=gamma)
        m = N if y is None else M
        assert node.shape == (N, m) and node.dtype == np.dtype(dtype)
        assert 'pairwise' not in be.calls  # lazy
        got = node.glom()
        if isinstance(hint, tuple):
          cuts = sorted({(e.ul[0], e.lr[0]) for e in x.val.tiles})
          assert sorted(be.pairwise_calls) == sorted((hi - lo, m, True, False, -1) for lo, hi in cuts)
          assert sorted((e.ul, e.lr) for e in node.force().tiles) == [((lo, 0), (hi, m)) for lo, hi in cuts]
        elif hint == 'replicated':
          assert be.pairwise_calls == [(N, m, True, False, -1)]
          assert isinstance(node.force(), distarray.ReplicatedArray)
        launches = be.calls.count('pairwise')
        assert launches >= 1 and np.array_equal(node.glom(), got) and be.calls.count('pairwise') == launches
        want = want_xx if y is None else want_xy
        assert got.dtype == np.dtype(dtype) and np.array_equal(got, want), (metric, hint, partner)


@pytest.mark.parametrize('W', [1, 2, 3, 4])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_normalized_affinity_every_layout(aff_ctx, W, dtype):
  import torch
  be = aff_ctx(W)
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from affinity_ref import affinity_ref, assert_within, points
  X = points(N, DIM, dtype, 3)
  L_ref, D_ref, A_ref, gs = affinity_ref(X, 'rbf', 0.3, 1.0)
  first = None
  for hint in HINTS:
    x = _operand(expr, distarray, torch, X, hint)
    del be.calls[:], be.pairwise_calls[:]
    L, D = expr.normalized_affinity(x, metric='rbf', gamma=0.3)
    assert L.shape == (N, N) and D.shape == (N,) and L.dtype == D.dtype == np.dtype(dtype)
    assert 'pairwise' not in be.calls  # lazy
    got_D = D.glom()
    launches = be.calls.count('pairwise')
    got_L = L.glom()
    assert be.calls.count('pairwise') == launches, hint  # the pair evaluated once
    if isinstance(hint, tuple):
      cuts = sorted({(e.ul[0], e.lr[0]) for e in x.val.tiles})
      # per row slab: the degree pass stores nothing, the scaled pass sets the slab's own diagonal
      assert sorted(be.pairwise_calls) == sorted([(hi - lo, N, False, True, -1) for lo, hi in cuts]
                                                 + [(hi - lo, N, True, False, lo) for lo, hi in cuts]), hint
      assert sorted((e.ul, e.lr) for e in L.force().tiles) == [((lo, 0), (hi, N)) for lo, hi in cuts]
      assert sorted((e.ul, e.lr) for e in D.force().tiles) == [((lo,), (hi,)) for lo, hi in cuts]
    elif hint == 'replicated':
      assert be.pairwise_calls == [(N, N, False, True, -1), (N, N, True, False, 0)]
      assert isinstance(L.force(), distarray.ReplicatedArray) and isinstance(D.force(), distarray.ReplicatedArray)
    assert got_L.dtype == got_D.dtype == np.dtype(dtype)
    assert np.all(np.diag(got_L) == 1.0) and np.array_equal(got_L, got_L.T)
    assert_within(got_D, D_ref, 0.0, dtype, ('D', hint))
    assert_within(got_L, L_ref, gs, dtype, ('L', hint), factor=2.0)
    if first is None:
      first = (got_L, got_D)
    assert np.array_equal(got_L, first[0]) and np.array_equal(got_D, first[1]), hint  # one answer for every layout
  # another diagonal, and a metric under which every degree of a duplicated point set is 0
  L, D = expr.normalized_affinity(X, metric='rbf', gamma=0.3, diagonal=0.5)
  assert np.all(np.diag(L.glom()) == 0.5)
  L, D = expr.normalized_affinity(np.ones((5, 2), dtype), metric='euclidean', diagonal=2.0)
  assert np.array_equal(D.glom(), np.zeros(5, dtype)) and np.array_equal(L.glom(), 2.0 * np.eye(5, dtype=dtype))


def test_refusals(aff_ctx):
  aff_ctx(1)
  import scipy.sparse as sp
  from spartan_amd import expr
  X, Y = np.ones((N, DIM)), np.ones((M, DIM))
  for fn in (expr.pairwise_kernel, expr.normalized_affinity):
    with pytest.raises(TypeError, match=r'todense\(\)'):
      fn(sp.csr_matrix(X))
    with pytest.raises(ValueError, match='2-d'):
      fn(np.ones(N))
    with pytest.raises(ValueError, match='2-d'):
      fn(np.ones((N, DIM, 1)))
    with pytest.raises(ValueError, match='no features'):
      fn(np.ones((N, 0)))
    with pytest.raises(ValueError, match='astype'):
      fn(X.astype(np.int64))
    with pytest.raises(ValueError, match='astype'):
      fn(X.astype(np.float16))
    with pytest.raises(ValueError, match="unknown metric 'cosine'"):
      fn(X, metric='cosine')
    with pytest.raises(ValueError, match='scaled_euclidean.*not built'):
      fn(X, metric='scaled_euclidean')
    for bad in (-1.0, float('nan'), float('inf')):
      with pytest.raises(ValueError, match='gamma'):
        fn(X, gamma=bad)
  with pytest.raises(TypeError, match=r'Y is a sparse.*todense\(\)'):
    expr.pairwise_kernel(X, sp.csr_matrix(Y))
  with pytest.raises(ValueError, match='Y must be 2-d'):
    expr.pairwise_kernel(X, np.ones(DIM))
  with pytest.raises(ValueError, match='X has 3 features and Y has 2'):
    expr.pairwise_kernel(X, np.ones((M, 2)))
  with pytest.raises(ValueError, match='one dtype.*astype'):
    expr.pairwise_kernel(X, Y.astype(np.float32))
  with pytest.raises(ValueError, match='diagonal'):
    expr.normalized_affinity(X, diagonal=float('nan'))
  # empty point sets are served, not refused
  assert expr.pairwise_kernel(np.ones((0, DIM)), Y).shape == (0, M)


# ------------------------------------------------------------------ driver
@pytest.mark.parametrize('W', [1, 3])
def test_driver_recovers_three_blobs(aff_ctx, W):
  be = aff_ctx(W)
  from spartan_amd import expr
  from spartan_amd.examples.spectral_clustering import spectral_cluster
  from affinity_ref import blobs, same_partition
  pts, truth = blobs(90, 2, 3)
  labels = spectral_cluster(expr.from_numpy(pts, tile_hint=(32, 2)), k=3, num_iter=5)
  got = labels.glom().reshape(-1)
  assert got.shape == (90,) and same_partition(got, truth)
  slabs = 3  # rows 0..32, 32..64, 64..90
  assert be.calls.count('pairwise') == 2 * slabs  # L is built once, not once a Lanczos step
  # a host array and the other metrics' names are taken too
  assert same_partition(spectral_cluster(pts, 3, 5, 'rbf').glom().reshape(-1), truth)


@pytest.mark.parametrize('metric', ['rbf', 'manhattan', 'euclidean'])
def test_driver_against_numpy_model(aff_ctx, metric):
  aff_ctx(2)
  from spartan_amd.examples.spectral_clustering import spectral_cluster
  from affinity_ref import blobs, spectral_model
  pts, _truth = blobs(45, 3, 3, seed=11, spread=0.5)
  want, _U, _init = spectral_model(pts, 3, 4, metric)
  got = spectral_cluster(pts, 3, 4, metric).glom().reshape(-1)
  assert np.array_equal(got, want), metric


# ------------------------------------------------------ the C ABI, no GPU
def _lib():
  import torch  # noqa: F401  (torch's HIP runtime first)
  from spartan_amd import binding
  return binding.load_library(), binding


@needs_lib
def test_plan_answers_without_gpu():
  lib, binding = _lib()
  for dtype in (np.float32, np.float64):
    tile, kc = binding.pairwise_plan(dtype, 1, 1)[:2]
    assert tile >= 16 and tile % 16 == 0 and 1 <= kc <= tile
    for n in (0, 1, 257, 2051, 1 << 13, 1 << 15, 1 << 20):
      t, k, splits, nbytes = binding.pairwise_plan(dtype, n, n)
      assert (t, k) == (tile, kc) and splits >= 1
      assert (nbytes == 0) == (splits == 1 or n == 0)
      if splits > 1:
        assert nbytes >= splits * n * 8  # float64 partials per split and row
        assert -(-n // tile) >= 4 * (splits - 1) + 1  # no range shorter than four tiles
    assert binding.pairwise_plan(dtype, 0, 100)[2:] == (1, 0) and binding.pairwise_plan(dtype, 100, 0)[2:] == (1, 0)
    # few rows against many columns are split; rows that fill the chip are not
    assert binding.pairwise_plan(dtype, tile, 1 << 17)[2] > 1
    assert binding.pairwise_plan(dtype, 1 << 20, 1 << 17)[2] == 1
    # forced splits are taken as they are, and the workspace is monotone in them
    sizes = [binding.pairwise_plan(dtype, 257, 257, s) for s in (1, 2, 3, 7, 64)]
    assert [s[2] for s in sizes] == [1, 2, 3, 7, 64]
    assert all(a[3] <= b[3] for a, b in zip(sizes, sizes[1:])) and sizes[0][3] == 0 < sizes[1][3]
    with pytest.raises(RuntimeError, match='splits'):
      binding.pairwise_plan(dtype, 257, 257, 1 << 20)
    with pytest.raises(RuntimeError, match='splits'):
      binding.pairwise_plan(dtype, 257, 257, -1)
  with pytest.raises(TypeError, match='float32 / float64'):
    binding.pairwise_plan(np.int32, 1, 1)
  for bad in ((-1, 1), (1, -1)):
    with pytest.raises(ValueError, match='negative size'):
      binding.pairwise_plan(np.float32, *bad)
  assert binding.PAIR_METRICS == {'sqeuclidean': 0, 'euclidean': 1, 'manhattan': 2, 'rbf': 3}
  # the library's own answers to what the wrapper refuses first
  t, k, s, b = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_size_t(0)
  args = (ctypes.byref(t), ctypes.byref(k), ctypes.byref(s), ctypes.byref(b))
  assert lib.spx_pairwise_plan(binding.SPX_I64, 1, 1, *args) == -3
  assert 'float32 / float64' in lib.spx_last_error().decode()
  assert lib.spx_pairwise_plan(9, 1, 1, *args) == -1 and 'bad dtype' in lib.spx_last_error().decode()
  assert lib.spx_pairwise_plan(binding.SPX_F32, -1, 1, *args) == -1 and 'negative size' in lib.spx_last_error().decode()
  assert lib.spx_pairwise_plan(binding.SPX_F64, 1, -5, *args) == -1 and 'negative size' in lib.spx_last_error().decode()
  assert lib.spx_pairwise_plan(binding.SPX_F64, 5, 5, None, None, None, None) == 0
  assert lib.spx_pairwise_plan(binding.SPX_F64, 1, 2 ** 63 - 1, *args) == -3 and 'm = ' in lib.spx_last_error().decode()
  assert lib.spx_pairwise_plan(binding.SPX_F64, 2 ** 63 - 1, 1, *args) == -3 and 'n = ' in lib.spx_last_error().decode()


@needs_lib
def test_argument_checks_without_gpu():
  lib, binding = _lib()
  F32, I64, EINVAL, ENOTSUP = binding.SPX_F32, binding.SPX_I64, -1, -3
  p = ctypes.c_void_p(4096)  # never dereferenced: every case fails its checks before any device work
  nul = ctypes.c_void_p(0)

  def call(dtype=F32, metric=3, n=5, m=7, d=3, X=p, ldx=3, Y=p, ldy=3, gamma=1.0, out=p, ldo=7, sums=nul, rs=nul,
           cs=nul, diag=-1, dval=0.0, splits=1, ws=nul, nws=0):
    return lib.spx_pairwise(dtype, metric, n, m, d, X, ldx, Y, ldy, gamma, out, ldo, sums, rs, cs, diag, dval, splits,
                            ws, ctypes.c_size_t(nws), nul)

  def err():
    return lib.spx_last_error().decode()

  assert call(dtype=I64) == ENOTSUP and 'float32 / float64' in err()
  assert call(dtype=9) == EINVAL and 'bad dtype' in err()
  assert call(n=-1) == EINVAL and 'negative size' in err()
  assert call(m=-1) == EINVAL and 'negative size' in err()
  for bad in (-1, 4, 99):
    assert call(metric=bad) == EINVAL and 'unknown metric' in err()
  for bad in (0, -3):
    assert call(d=bad) == EINVAL and 'd = ' in err()
  for bad in (-1.0, float('nan'), float('inf')):
    assert call(gamma=bad) == EINVAL and 'gamma' in err()
  assert call(out=nul, sums=nul) == EINVAL and 'both NULL' in err()
  assert call(rs=p) == EINVAL and 'go together' in err()
  assert call(cs=p) == EINVAL and 'go together' in err()
  assert call(ldx=2) == EINVAL and 'ldx' in err()
  assert call(ldy=2) == EINVAL and 'ldy' in err()
  assert call(ldo=6) == EINVAL and 'ldo' in err()
  assert call(X=nul) == EINVAL and 'null pointer' in err()
  assert call(Y=nul) == EINVAL and 'null pointer' in err()
  assert call(splits=-1) == EINVAL and 'splits' in err()
  assert call(splits=1 << 20) == EINVAL and 'splits' in err()
  # a forced split of the row sums above what the workspace holds
  need = binding.pairwise_plan(np.float32, 5, 7, 3)[3]
  assert need > 0
  assert call(sums=p, splits=3, ws=nul, nws=0) == EINVAL and 'workspace' in err()
  assert call(sums=p, splits=3, ws=p, nws=need - 1) == EINVAL and 'workspace' in err()
  assert call(sums=p, splits=3, ws=ctypes.c_void_p(4097), nws=need) == EINVAL and 'aligned' in err()
  # no rows or no columns: nothing is looked at, nothing is launched
  assert call(n=0, X=nul, Y=nul) == 0
  assert call(m=0, X=nul, Y=nul, ldo=0) == 0


@needs_lib
def test_backend_wrapper_checks_without_gpu():
  """HipBackend.pairwise names the offending argument before any call."""
  import torch
  from spartan_amd import backend
  be = backend.HipBackend.__new__(backend.HipBackend)
  be._pairwise_ws = {}
  X = torch.zeros((5, 3), dtype=torch.float32)
  Y = torch.zeros((7, 3), dtype=torch.float32)

  def call(X=X, Y=Y, metric='rbf', gamma=1.0, **kw):
    kw.setdefault('out', True)
    return be.pairwise(X, Y, metric, gamma, **kw)

  with pytest.raises(ValueError, match='X must be 2-d'):
    call(X=torch.zeros((5,), dtype=torch.float32))
  with pytest.raises(ValueError, match='Y must be 2-d'):
    call(Y=torch.zeros((7, 3, 1), dtype=torch.float32))
  with pytest.raises(ValueError, match='X must be float32 / float64'):
    call(X=X.to(torch.int64))
  with pytest.raises(ValueError, match='Y has dtype'):
    call(Y=Y.to(torch.float64))
  with pytest.raises(ValueError, match='Y has 2 features, X has 3'):
    call(Y=torch.zeros((7, 2), dtype=torch.float32))
  with pytest.raises(ValueError, match='no features'):
    call(X=torch.zeros((5, 0), dtype=torch.float32), Y=torch.zeros((7, 0), dtype=torch.float32))
  with pytest.raises(ValueError, match="metric 'cosine'"):
    call(metric='cosine')
  with pytest.raises(ValueError, match='gamma'):
    call(gamma=-1.0)
  with pytest.raises(ValueError, match='X must have unit column stride'):
    call(X=torch.zeros((3, 5), dtype=torch.float32).t())
  with pytest.raises(ValueError, match='row_scale and col_scale go together'):
    call(row_scale=torch.zeros((5,), dtype=torch.float32))
  with pytest.raises(ValueError, match='pairwise: col_scale must be'):
    call(row_scale=torch.zeros((5,), dtype=torch.float32), col_scale=torch.zeros((5,), dtype=torch.float32))
  with pytest.raises(ValueError, match='pairwise: row_scale must be'):
    call(row_scale=torch.zeros((5,), dtype=torch.float64), col_scale=torch.zeros((7,), dtype=torch.float32))
  with pytest.raises(ValueError, match='out must be a \\(5, 7\\)'):
    call(out=torch.zeros((5, 6), dtype=torch.float32))
  with pytest.raises(ValueError, match='pairwise: row_sums must be'):
    call(row_sums=torch.zeros((4,), dtype=torch.float32))
  with pytest.raises(ValueError, match='neither out nor row_sums'):
    call(out=None)
  with pytest.raises(ValueError, match='diag_col0'):
    call(diag_col0=-2)
  with pytest.raises(ValueError, match='splits'):
    call(splits=-2)
  # no rows / no columns: no call into the library; the sums of nothing are zeros
  out, sums = call(X=torch.zeros((0, 3), dtype=torch.float32), row_sums=True)
  assert out.shape == (0, 7) and sums.shape == (0,)
  out, sums = call(Y=torch.zeros((0, 3), dtype=torch.float32), row_sums=torch.ones((5,), dtype=torch.float32))
  assert out.shape == (5, 0) and torch.equal(sums, torch.zeros((5,), dtype=torch.float32))

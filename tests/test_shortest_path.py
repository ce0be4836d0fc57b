"""``spartan_amd.shortest_path`` and ``examples.isomap.Isomap`` host logic (no
GPU): every route of the expression layer over tile layouts and worker counts,
sparse and dense operands, laziness, validation, the ``info`` error, the
``unreachable`` value, the plan / no-launch answers of spx_apsp, the
yardstick's own cross-check, and the Isomap driver against its NumPy model.

The expression layer runs here over the CPU test double whose ``apsp`` is the
yardstick (graph_ref.GraphFakeBackend); the kernels themselves are tested on
the GPU in tests/test_shortest_path_gpu.py.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, 'spartan_amd', 'libspx.so')

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')

N = 10
HINTS = [(10, 10), (4, 10), (10, 3), (4, 3)]


@pytest.fixture
def graph_ctx(host_ctx):
  """host_ctx with the shortest-path-capable test double installed."""
  from spartan_amd import backend
  from graph_ref import GraphFakeBackend

  def make(num_workers=1):
    host_ctx(num_workers)
    be = GraphFakeBackend()
    backend.set_backend(be)
    return be
  return make


@pytest.fixture
def gathers(monkeypatch):
  """Counts the ``gather_regions`` exchanges."""
  from spartan_amd.array import distarray
  calls = []
  real = distarray.gather_regions

  def counted(array, requests):
    calls.append(len(requests))
    return real(array, requests)
  monkeypatch.setattr(distarray, 'gather_regions', counted)
  return calls


def _same_bits(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _graph(dtype, seed=3):
  """(10, 10): a sparse random digraph with some unreachable pairs."""
  r = np.random.RandomState(seed)
  G = np.where(r.rand(N, N) < 0.2, r.randint(1, 50, size=(N, N)), 0).astype(dtype)
  G[np.arange(N), np.arange(N)] = 0
  return G


# --------------------------------------------------------------- yardstick
@pytest.mark.parametrize('kind', ['int', 'knn', 'chain', 'empty'])
@pytest.mark.parametrize('directed', [True, False])
def test_yardstick_against_plain_floyd_warshall(kind, directed):
  """scipy's Dijkstra and n NumPy passes agree: exactly on integer weights,
  to rounding (different association of the same sums) on real ones."""
  from graph_ref import apsp_ref, fw_numpy, graph_data
  for n in (1, 2, 17, 65):
    for dtype in (np.float32, np.float64):
      G = graph_data(kind, n, dtype, seed=n)
      ref, fw = apsp_ref(G, directed), fw_numpy(G, directed)
      assert np.array_equal(np.isinf(ref), np.isinf(fw))
      fin = np.isfinite(ref)
      if kind in ('int', 'chain', 'empty'):
        assert np.array_equal(ref[fin], fw[fin])
      else:
        np.testing.assert_allclose(ref[fin], fw[fin], rtol=1e-14)
  G = graph_data('int', 17, np.float64, seed=1)
  assert np.array_equal(apsp_ref(G, True, 7.5) == 7.5, np.isinf(apsp_ref(G, True)))


# ------------------------------------------------------------- expr layer
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_shortest_path_every_route(graph_ctx, gathers, W, dtype):
  import scipy.sparse as sp
  import torch
  be = graph_ctx(W)
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from graph_ref import apsp_ref
  G = _graph(dtype)
  for directed in (True, False):
    want = apsp_ref(G, directed).astype(dtype)
    assert np.isinf(want).any() and np.isfinite(want).sum() > N
    for hint in HINTS + ['replicated', 'host', 'sparse', 'sparse-slabs']:
      if hint == 'replicated':
        x = expr.lazify(distarray.ReplicatedArray(torch.as_tensor(G.copy())))
      elif hint == 'host':
        x = G
      elif hint == 'sparse':
        x = expr.from_numpy(sp.csr_matrix(G))
      elif hint == 'sparse-slabs':
        x = expr.from_numpy(sp.csr_matrix(G), tile_hint=(4, N))
      else:
        x = expr.lazify(expr.from_numpy(G, tile_hint=hint).force())
      del be.calls[:]
      del gathers[:]
      node = expr.shortest_path(x, directed=directed)
      assert node.shape == (N, N) and node.dtype == np.dtype(dtype)
      out = node.force()
      assert be.calls.count('apsp') == 1, hint
      if hint == 'replicated':
        assert isinstance(out, distarray.ReplicatedArray) and not gathers
      elif isinstance(hint, tuple):
        assert out.tiles == x.val.tiles, hint  # the input's tiling
        assert len(gathers) == (0 if len(out.tiles) == 1 else 1), hint  # ONE exchange of the whole matrix
      elif hint == 'sparse-slabs':
        cuts = sorted((e.ul[0], e.lr[0]) for e in x.val.tiles)
        assert sorted((e.ul[0], e.lr[0]) for e in out.tiles) == cuts  # row slabs at the input's row cuts
        assert all(e.ul[1] == 0 and e.lr[1] == N for e in out.tiles)
      assert _same_bits(out.glom(), want), hint  # the same bits for every layout


def test_lazy_until_forced(graph_ctx):
  be = graph_ctx(3)
  from spartan_amd import expr
  G = _graph(np.float64)
  node = expr.shortest_path(expr.from_numpy(G, tile_hint=(4, 3)), directed=False)
  twice = node + node
  assert isinstance(node, expr.Expr) and 'apsp' not in be.calls
  a = node.glom()
  assert be.calls.count('apsp') == 1
  assert np.array_equal(twice.glom(), 2 * a) and be.calls.count('apsp') == 1


def test_validation_errors(graph_ctx):
  graph_ctx(1)
  import scipy.sparse as sp
  from spartan_amd import expr
  for bad in (np.ones(4), np.ones((3, 4)), np.ones((2, 3, 3)), sp.csr_matrix(np.ones((3, 4)))):
    with pytest.raises(ValueError, match='square'):
      expr.shortest_path(bad)
  with pytest.raises(TypeError, match='float32 / float64'):
    expr.shortest_path(np.ones((4, 4), np.int64))
  for bad in (-1.0, float('nan'), -np.inf):
    with pytest.raises(ValueError, match='unreachable'):
      expr.shortest_path(np.ones((4, 4)), unreachable=bad)


@pytest.mark.parametrize('W', [1, 3])
def test_bad_weight_raises_on_evaluation(graph_ctx, W):
  graph_ctx(W)
  from spartan_amd import expr
  for bad in (-1.0, float('nan'), -np.inf):
    G = _graph(np.float64)
    G[2, 5] = bad
    for hint in ((10, 10), (4, 3)):
      node = expr.shortest_path(expr.from_numpy(G, tile_hint=hint))  # lazily: no error yet
      with pytest.raises(ValueError, match='shortest_path: negative or NaN edge weight'):
        node.force()


def test_unreachable_value_and_edge_rules(graph_ctx):
  graph_ctx(1)
  from spartan_amd import expr
  from graph_ref import apsp_ref
  G = _graph(np.float32)
  inf = expr.shortest_path(G).glom()
  for value in (0.0, 1e6):
    got = expr.shortest_path(G, unreachable=value).glom()
    assert np.array_equal(got == np.float32(value), np.isinf(inf) | (inf == np.float32(value)))
    assert np.array_equal(got[np.isfinite(inf)], inf[np.isfinite(inf)])
  H = G.copy()
  H[H == 0] = np.inf                      # +inf is "no edge" as 0 is
  H[np.arange(N), np.arange(N)] = 123.0   # the diagonal is ignored
  assert _same_bits(expr.shortest_path(H).glom(), inf)
  assert _same_bits(inf, apsp_ref(G).astype(np.float32))


# ------------------------------------------------------------------ the ABI
@needs_lib
def test_apsp_plan_and_no_launch_cases():
  """Every argument check of spx_apsp / spx_apsp_plan returns its code and
  message without any device work."""
  from spartan_amd import backend
  lib = backend.load_library()
  EINVAL, ENOTSUP = -1, -3
  err = lib.spx_last_error
  for dt, code in ((np.float32, 3), (np.float64, 4)):
    b = backend.apsp_plan(dt)
    assert b >= 16 and b % 4 == 0
    tile = ctypes.c_int64(0)
    assert lib.spx_apsp_plan(code, ctypes.byref(tile)) == 0 and tile.value == b
    assert lib.spx_apsp(code, 1, 0, None, 0, None, 0, np.inf, None, None) == 0  # n == 0: no pointer is looked at
  with pytest.raises(TypeError):
    backend.apsp_plan(np.int32)
  assert lib.spx_apsp_plan(1, None) == ENOTSUP and lib.spx_apsp_plan(99, None) == EINVAL
  assert lib.spx_apsp_plan(3, None) == 0
  g = ctypes.c_void_p(0x1000)  # never dereferenced: every case below is refused before a launch
  d = ctypes.c_void_p(0x2000)
  info = ctypes.c_void_p(0x3000)

  def apsp(dt=4, directed=1, n=4, G=g, ldg=4, D=d, ldd=4, unreachable=np.inf, inf=info):
    return lib.spx_apsp(dt, directed, n, G, ldg, D, ldd, unreachable, inf, None)
  assert apsp(dt=99) == EINVAL and b'dtype' in err()
  assert apsp(dt=-1) == EINVAL and b'dtype' in err()
  assert apsp(dt=2) == ENOTSUP and b'float32 / float64' in err()
  assert apsp(n=-1) == EINVAL and b'negative' in err()
  for name in ('G', 'D', 'inf'):
    assert apsp(**{name: None}) == EINVAL and b'null' in err()
  assert apsp(ldg=3) == EINVAL and b'leading dimension' in err()
  assert apsp(ldd=3) == EINVAL and b'leading dimension' in err()
  assert apsp(D=g) == EINVAL and b'D may not be G' in err()
  assert apsp(unreachable=-1.0) == EINVAL and b'unreachable' in err()
  assert apsp(unreachable=float('nan')) == EINVAL and b'unreachable' in err()


def test_hipbackend_apsp_rejects_malformed_tensors():
  """HipBackend.apsp validates as syevj does, before the library sees anything."""
  import torch
  from spartan_amd import backend
  be = backend.HipBackend.__new__(backend.HipBackend)  # no library, no device: only the checks run
  with pytest.raises(ValueError, match='2-d'):
    be.apsp(torch.ones(4))
  with pytest.raises(ValueError, match='square'):
    be.apsp(torch.ones(3, 4))
  with pytest.raises(ValueError, match='float32 / float64'):
    be.apsp(torch.ones(4, 4, dtype=torch.int64))
  with pytest.raises(ValueError, match='unit stride'):
    be.apsp(torch.ones(4, 8).t()[:4, :4])
  with pytest.raises(ValueError, match='unit stride'):
    be.apsp(torch.ones(4, 8)[:, ::2])
  with pytest.raises(ValueError, match='unreachable'):
    be.apsp(torch.ones(4, 4), unreachable=-1.0)
  D, info = be.apsp(torch.ones(0, 0))
  assert tuple(D.shape) == (0, 0) and int(info[0]) == 0


# ------------------------------------------------------------------- Isomap
ISO_N, ISO_K, ISO_TOL = 150, 8, 1e-8


@pytest.fixture(scope='module')
def iso_model():
  from graph_ref import isomap_model, swiss_roll
  X = swiss_roll(ISO_N, seed=0)
  return X, isomap_model(X, ISO_K, 2)


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_isomap_against_the_numpy_model(graph_ctx, iso_model, W):
  be = graph_ctx(W)
  from spartan_amd.examples.isomap import Isomap
  from graph_ref import check_isomap
  X, model = iso_model
  iso = Isomap(n_neighbors=ISO_K, n_components=2, tol=ISO_TOL).fit(X)
  assert be.calls.count('apsp') == 1
  assert isinstance(iso.embedding_, np.ndarray) and isinstance(iso.dist_matrix_, np.ndarray)
  assert iso.embedding_.shape == (ISO_N, 2) and iso.dist_matrix_.shape == (ISO_N, ISO_N)
  assert iso.training_data_ is X
  assert 0 < iso.n_iter_ < 200
  check_isomap(model, iso, ISO_TOL, 'isomap W=%d' % W)


@needs_lib
def test_isomap_dense_solver(graph_ctx):
  graph_ctx(1)
  from spartan_amd.examples.isomap import Isomap
  from graph_ref import check_isomap, isomap_model, swiss_roll
  X = swiss_roll(60, seed=0)
  model = isomap_model(X, ISO_K, 2)
  dense = Isomap(n_neighbors=ISO_K, n_components=2, eigen_solver='dense').fit(X)
  assert dense.n_iter_ == 0
  check_isomap(model, dense, ISO_TOL, 'isomap dense')
  it = Isomap(n_neighbors=ISO_K, n_components=2, eigen_solver='arpack', tol=ISO_TOL).fit(X)
  check_isomap(model, it, ISO_TOL, 'isomap arpack n=60')
  with pytest.raises(NotImplementedError, match='dense'):
    Isomap(n_neighbors=ISO_K, eigen_solver='dense').fit(swiss_roll(100, seed=0))


@needs_lib
def test_isomap_errors(graph_ctx):
  graph_ctx(1)
  from spartan_amd import backend
  from spartan_amd.examples.isomap import Isomap
  from graph_ref import swiss_roll
  r = np.random.RandomState(0)
  two = np.concatenate([r.rand(20, 3), r.rand(20, 3) + 100.0])  # two far clusters
  with pytest.raises(ValueError, match=r'not connected: 800 pairs .* n_neighbors = 5'):
    Isomap(n_neighbors=5).fit(two)
  X = swiss_roll(40, seed=0)
  with pytest.raises(ValueError, match='KNN_K_MAX'):
    Isomap(n_neighbors=backend.KNN_K_MAX).fit(X)
  with pytest.raises(ValueError, match='exceeds the 40 fitted points'):
    Isomap(n_neighbors=40).fit(X)
  with pytest.raises(ValueError, match='columns are iterated'):
    Isomap(n_neighbors=5, n_components=33).fit(X)
  with pytest.raises(ValueError, match='eigen_solver'):
    Isomap(eigen_solver='lobpcg')
  # duplicate points: their zero-length edge vanishes, the graph stays connected through the others
  dup = X.copy()
  dup[1] = dup[0]
  iso = Isomap(n_neighbors=8, tol=1e-8).fit(dup)
  assert np.isfinite(iso.dist_matrix_).all() and iso.dist_matrix_[0, 1] > 0


@needs_lib
def test_isomap_says_when_the_rounds_run_out(graph_ctx):
  graph_ctx(1)
  from spartan_amd.examples.isomap import Isomap
  from graph_ref import swiss_roll
  X = swiss_roll(60, seed=0)
  with pytest.warns(RuntimeWarning, match=r'spent its 1 rounds'):
    short = Isomap(n_neighbors=ISO_K, tol=1e-12, max_iter=1).fit(X)
  assert short.n_iter_ == 1 and short.converged_ is False and short.embedding_.shape == (60, 2)
  with warnings.catch_warnings():
    warnings.filterwarnings('error', message='Isomap')
    done = Isomap(n_neighbors=ISO_K, tol=ISO_TOL).fit(X)
  assert done.converged_ is True and 0 < done.n_iter_ < 200
  assert Isomap(n_neighbors=ISO_K, eigen_solver='dense').fit(X).converged_ is True

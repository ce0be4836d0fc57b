"""Sparse arrays and the sparse expression layer, host logic (no GPU): ingest
and ``glom`` over tile layouts and worker counts, the constructors, ``dot`` /
``todense`` / ``sum`` / scaling, every refusal, two gloo ranks, the PageRank and
conjugate-gradient drivers, and the plan / workspace answers and argument
checks of spx_csrmm / spx_csr_todense.

The expression layer runs here over the CPU test double with scipy ``csrmm`` /
``csr_todense`` (sparse_ref.SparseFakeBackend); the kernels themselves are
tested on the GPU in tests/test_sparse_gpu.py.
"""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, 'spartan_amd', 'libspx.so')

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')

M, N = 23, 17
# default slabs; one tile; several slabs per worker; one row per slab (more slabs than rows that hold data, see
# _tail_empty); a hint wider than the matrix
HINTS = [None, (M, N), (5, N), (1, N), (4, N + 3)]
WS = [1, 3]


@pytest.fixture
def sparse_ctx(host_ctx):
  """host_ctx with the sparse-capable test double installed."""
  from spartan_amd import backend
  from sparse_ref import SparseFakeBackend

  def make(num_workers=1):
    host_ctx(num_workers)
    be = SparseFakeBackend()
    backend.set_backend(be)
    return be
  return make


def _same_csr(got, want):
  import scipy.sparse as sp
  from sparse_ref import same_bits
  assert sp.isspmatrix_csr(got) and got.shape == want.shape and got.dtype == want.dtype
  assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
  assert same_bits(got.data, want.data)


def _tail_empty(dtype):
  """Data in the first 4 rows only: at one row per slab most slabs hold only empty rows."""
  import scipy.sparse as sp
  from sparse_ref import sparse_data
  return sp.vstack([sparse_data('uniform', 4, N, dtype, L=5), sp.csr_matrix((M - 4, N), dtype=dtype)]).tocsr()


def _matrices(dtype):
  from sparse_ref import KINDS, sparse_data
  out = [(k, sparse_data(k, M, 1 if k == 'onecol' else N, dtype)) for k in KINDS]
  out.append(('tail_empty', _tail_empty(dtype)))
  return out


# ------------------------------------------------------------------ ingest
@needs_lib
@pytest.mark.parametrize('W', WS)
@pytest.mark.parametrize('hint', HINTS)
def test_from_scipy_glom_roundtrip(sparse_ctx, W, hint):
  sparse_ctx(W)
  import scipy.sparse as sp
  from spartan_amd import expr
  from spartan_amd.array import sparse as sparray
  for dtype in (np.float32, np.float64):
    for kind, A in _matrices(dtype):
      h = hint  # wider than a one-column matrix too: a hint may exceed the shape
      for fmt in ('csr', 'csc', 'coo', 'lil'):
        S = sparray.from_scipy(A.asformat(fmt), tile_hint=h)
        assert S.sparse and S.shape == A.shape and S.dtype == dtype and S.nnz == A.nnz
        assert all(e.ul[1] == 0 and e.lr[1] == A.shape[1] for e in S.tiles)
        if h == (1, N):
          assert len(S.tiles) == M and {w for w in S.tiles.values()} == set(range(W))
        _same_csr(S.glom(), A)
      _same_csr(expr.from_numpy(A, tile_hint=h).glom(), A)
  # duplicate and unsorted coo entries: summed and sorted on the host
  rows = np.array([3, 0, 3, 22, 3, 0, 7])
  cols = np.array([5, 16, 5, 0, 2, 16, 7])
  vals = np.array([1.5, 2.0, 0.25, -3.0, 4.0, 8.0, 0.5], np.float32)
  coo = sp.coo_matrix((vals, (rows, cols)), shape=(M, N))
  want = coo.tocsr()
  want.sum_duplicates()
  want.sort_indices()
  for h in HINTS:
    S = sparray.from_scipy(coo, tile_hint=h)
    assert S.nnz == 5
    _same_csr(S.glom(), want)
  assert coo.nnz == 7  # the caller's matrix is not canonicalised in place


@needs_lib
def test_ingest_entry_points_and_layout_errors(sparse_ctx):
  sparse_ctx(3)
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from spartan_amd.array import sparse as sparray
  from sparse_ref import sparse_data
  A = sparse_data('uniform', M, N, np.float32)
  for e in (expr.from_numpy(A), expr.lazify(A), expr.as_array(A), expr.lazify(sparray.from_scipy(A))):
    assert e.sparse_result and isinstance(e.force(), sparray.SparseDistArray)
    _same_csr(e.glom(), A)
  # the default layout deals the rows evenly to the workers, round robin
  S = expr.from_numpy(A).force()
  assert sorted((e.ul[0], e.lr[0], w) for e, w in S.tiles.items()) == [(0, 8, 0), (8, 16, 1), (16, 23, 2)]
  want = distarray.compute_extents((M, N), (5, N), 3)
  assert expr.from_numpy(A, tile_hint=(5, N)).force().tiles == want
  with pytest.raises(NotImplementedError, match='row slabs'):
    sparray.from_scipy(A, tile_hint=(M, 4))
  with pytest.raises(NotImplementedError, match='row slabs'):
    expr.sparse_rand((M, N), density=0.1, tile_hint=(5, 5)).force()
  with pytest.raises(TypeError, match='float32 / float64'):
    sparray.from_scipy(A.astype(np.int32))
  with pytest.raises(TypeError):
    sparray.from_scipy(A.toarray())
  with pytest.raises(TypeError, match='immutable'):
    S.update(None, None)


@needs_lib
@pytest.mark.parametrize('W', WS)
def test_constructors(sparse_ctx, W):
  sparse_ctx(W)
  import scipy.sparse as sp
  from spartan_amd import expr
  for dtype in (np.float32, np.float64):
    want = sp.random(40, 30, density=0.1, format='csr', dtype=dtype, random_state=np.random.RandomState(3))
    for hint in (None, (40, 30), (7, 30), (1, 30)):
      e = expr.sparse_rand((40, 30), density=0.1, dtype=dtype, tile_hint=hint, seed=3)
      assert e.shape == (40, 30) and e.dtype == dtype
      _same_csr(e.glom(), want)
      _same_csr(expr.sparse_rand((40, 30), density=0.1, format='coo', dtype=dtype, tile_hint=hint, seed=3).glom(),
                want)
    for shape in ((9, 9), (5, 9), (9, 5), (1, 4), (4, 1)):
      for hint in (None, (2, shape[1]), (1, shape[1])):
        d = expr.sparse_diagonal(shape, dtype=dtype, tile_hint=hint)
        _same_csr(d.glom(), sp.eye(shape[0], shape[1], dtype=dtype, format='csr'))
        assert d.force().nnz == min(shape)
        z = expr.sparse_empty(shape, dtype=dtype, tile_hint=hint)
        assert z.force().nnz == 0
        _same_csr(z.glom(), sp.csr_matrix(shape, dtype=dtype))
  a = expr.sparse_rand((40, 30), density=0.1).glom()  # an unseeded draw differs from the next one
  b = expr.sparse_rand((40, 30), density=0.1).glom()
  assert a.dtype == np.float32 and (a != b).nnz > 0
  with pytest.raises(TypeError):
    expr.sparse_diagonal((4, 4), dtype=np.int32)
  with pytest.raises(ValueError):
    expr.sparse_empty((4,))


# --------------------------------------------------------------------- dot
@needs_lib
@pytest.mark.parametrize('W', WS)
@pytest.mark.parametrize('hint', HINTS)
def test_dot(sparse_ctx, W, hint):
  be = sparse_ctx(W)
  from spartan_amd import expr
  from sparse_ref import assert_within, dense_data
  for sd in (np.float32, np.float64):
    for kind, A in _matrices(sd):
      n = A.shape[1]
      S = expr.from_numpy(A, tile_hint=hint)
      Sa = S.force()
      for xd in (np.float32, np.float64):
        for shape in ((n,), (n, 1), (n, 4)):
          X = dense_data(n, shape[-1] if len(shape) == 2 else 1, xd).reshape(shape)
          Xe = expr.from_numpy(X, tile_hint=(3,) + shape[1:])
          for operand in (X, Xe, Xe.force()):
            del be.calls[:]
            y = expr.dot(S, operand)
            want = A.dot(X)
            assert y.shape == want.shape and y.dtype == want.dtype == np.result_type(sd, xd)
            ya = y.force()
            assert be.calls.count('csrmm') == len(Sa.tiles)
            # the output's tiling: S's slabs on the same workers
            assert {(e.ul[0], e.lr[0]): w for e, w in ya.tiles.items()} == \
                {(e.ul[0], e.lr[0]): w for e, w in Sa.tiles.items()}
            assert all(len(e.shape) == len(shape) and e.shape[1:] == want.shape[1:] for e in ya.tiles)
            got = ya.glom()
            assert got.shape == want.shape and got.dtype == want.dtype
            wide = A.astype(want.dtype)
            X2 = X.reshape(n, -1).astype(want.dtype)
            assert_within(got.reshape(M, -1), wide, X2, np.zeros((M, X2.shape[1]), want.dtype), 1.0, 0.0,
                          'dot %s %s' % (kind, shape))
  for bad in (np.ones(N + 1), np.ones((N + 1, 2)), np.ones((1, N))):
    with pytest.raises(ValueError):
      expr.dot(expr.from_numpy(_tail_empty(np.float32)), bad)  # at construction
  # an integer dense operand computes in float64 (NumPy's result type)
  Xi = np.arange(N, dtype=np.int64)
  A = _tail_empty(np.float32)
  y = expr.dot(expr.from_numpy(A), Xi)
  assert y.dtype == np.float64 and np.array_equal(y.glom(), A.astype(np.float64).dot(Xi))


@needs_lib
def test_issue_example(sparse_ctx):
  sparse_ctx(3)
  import scipy.sparse as sp
  from spartan_amd import expr
  from sparse_ref import assert_within
  got = expr.dot(expr.sparse_rand((1000, 1000), density=0.01, seed=1), expr.ones((1000, 1))).glom()
  A = sp.random(1000, 1000, density=0.01, format='csr', dtype=np.float32, random_state=np.random.RandomState(1))
  assert got.dtype == np.float64  # ones defaults to float64
  A64 = A.astype(np.float64)
  assert_within(got, A64, np.ones((1000, 1)), np.zeros((1000, 1)), 1.0, 0.0, 'issue example')


# ------------------------------------------- todense, sum, scaling, nnz
@needs_lib
@pytest.mark.parametrize('W', WS)
@pytest.mark.parametrize('hint', HINTS)
def test_todense_sum_scale_nnz(sparse_ctx, W, hint):
  sparse_ctx(W)
  from spartan_amd import expr
  from sparse_ref import LD, assert_within, same_bits, unit_roundoff
  for dtype in (np.float32, np.float64):
    for kind, A in _matrices(dtype):
      n = A.shape[1]
      S = expr.from_numpy(A, tile_hint=hint)
      for d in (expr.todense(S), S.todense()):
        da = d.force()
        assert not da.sparse and da.tiles == S.force().tiles
        assert same_bits(d.glom(), A.toarray())
      assert same_bits((d + 1).glom(), A.toarray() + 1)  # a dense array like any other
      r = expr.sum(S, axis=1)
      assert r.shape == (M,) and r.dtype == dtype
      ones = np.ones((n, 1), dtype)
      assert_within(r.glom().reshape(M, 1), A, ones, np.zeros((M, 1), dtype), 1.0, 0.0, 'sum axis 1 %s' % kind)
      assert same_bits(S.sum(axis=1).glom(), r.glom())
      t = expr.sum(S)
      u = unit_roundoff(dtype)
      k = int(np.diff(A.indptr).max()) + 2 + (M - 1)
      assert t.shape == () or t.shape == (1,) or t.shape == tuple(np.shape(t.glom()))
      assert abs(LD(float(t.glom())) - A.data.astype(LD).sum()) <= (k * u / (1 - k * u)) * np.abs(A.data).astype(LD).sum()
      with pytest.raises(NotImplementedError, match='transpose'):
        expr.sum(S, axis=0)
      for c in (2.5, 3, np.float32(-0.5), np.float64(0.0)):
        for sc in (S * c, c * S):
          assert sc.sparse_result and sc.dtype == dtype and sc.shape == A.shape
          want = A.copy()
          want.data = (want.data * dtype(c)).astype(dtype)
          _same_csr(sc.glom(), want)  # the same structure, explicit zeros included
      assert S.force().nnz == A.nnz and (S * 2).force().nnz == A.nnz


# --------------------------------------------------------------- refusals
@needs_lib
def test_refusals(sparse_ctx):
  be = sparse_ctx(3)
  from spartan_amd import expr
  from sparse_ref import sparse_data
  A = sparse_data('uniform', M, N, np.float32)
  S = expr.from_numpy(A, tile_hint=(5, N))
  Sa = S.force()
  D = expr.ones((M, N), dtype=np.float32)
  sq = expr.from_numpy(sparse_data('uniform', N, N, np.float32))
  del be.calls[:]
  cases = {
      'S + D': lambda: (S + D).force(), 'D + S': lambda: (D + S).force(), 'S * D': lambda: (S * D).force(),
      'D * S': lambda: (D * S).force(), 'S + 1': lambda: (S + 1).force(), 'S / 2': lambda: (S / 2).force(),
      '-S': lambda: (-S).force(), 'S * S': lambda: (S * S).force(), 'exp': lambda: expr.exp(S).force(),
      'slice': lambda: S[0:2].force(), 'int index': lambda: S[0].force(), 'T': lambda: S.T.force(),
      'transpose': lambda: expr.transpose(S).force(), 'reshape': lambda: expr.reshape(S, (N, M)).force(),
      'dot(D, S)': lambda: expr.dot(expr.ones((4, M), dtype=np.float32), S).force(),
      'dot(ndarray, S)': lambda: expr.dot(np.ones((4, M), np.float32), S).force(),
      'dot(S, S)': lambda: expr.dot(S, sq).force(), 'dot(S, scipy)': lambda: expr.dot(S, sq.glom()).force(),
      'max': lambda: expr.max(S).force(), 'mean': lambda: expr.mean(S).force(),
      'argmax': lambda: expr.argmax(S, axis=1).force(), 'sort': lambda: expr.sort(S).force(),
      'scan': lambda: expr.scan(S, axis=0).force(), 'forced + D': lambda: (expr.lazify(Sa) + D).force(),
      'fetch': lambda: Sa.fetch(list(Sa.tiles)[0]), 'getitem': lambda: Sa[0:2],
      'from Val': lambda: (expr.base.Val(val=Sa) + D).force(),
  }
  for name, fn in cases.items():
    with pytest.raises(TypeError, match='todense'):
      fn()
      pytest.fail('%s was accepted' % name)
  assert not be.calls, 'a refusal ran device work: %s' % be.calls  # nothing densified silently


# --------------------------------------------------------------- drivers
def _spd(n, dtype=np.float64, seed=2):
  """A = s I + (B + B^T) with s twice the largest off-diagonal absolute row
  sum: Gershgorin puts the spectrum in [s/2, 3s/2], cond <= 3."""
  import scipy.sparse as sp
  B = sp.random(n, n, density=0.03, format='csr', dtype=dtype, random_state=np.random.RandomState(seed))
  Bs = (B + B.T).tocsr()
  Bs.setdiag(0)
  Bs.eliminate_zeros()
  s = 2 * abs(Bs).sum(1).max()
  return (s * sp.eye(n, dtype=dtype) + Bs).tocsr()


def _pagerank_ref(W, T, damping=0.85):
  """The iteration of examples/pagerank.py in np.longdouble on the float32
  matrix ``W`` (scipy CSR), with the float32 constants the driver uses."""
  from sparse_ref import LD
  n = W.shape[1]
  p = np.full((n, 1), LD(np.float32(1.0 / n)))
  for _ in range(T):
    p = LD(np.float32(damping)) * _ld_matvec(W, p) + LD(np.float32((1.0 - damping) / n))
  return p


def _ld_matvec(W, p):
  out = np.zeros((W.shape[0], 1), np.longdouble)
  data = W.data.astype(np.longdouble)
  for i in range(W.shape[0]):
    a, b = W.indptr[i], W.indptr[i + 1]
    out[i, 0] = (data[a:b] * p[W.indices[a:b], 0]).sum()
  return out


def _check_pagerank(Wm, T):
  from spartan_amd.examples.pagerank import pagerank
  from sparse_ref import LD, unit_roundoff
  ref = Wm.glom()
  want = _pagerank_ref(ref, T)
  got = pagerank(Wm, num_iter=T).glom()
  assert got.shape == want.shape and got.dtype == np.float32
  kmax = int(np.diff(ref.indptr).max())
  # all terms are non-negative, so relative errors only add: (kmax + 2) roundings per iteration and entry
  assert np.all(np.abs(got.astype(LD) - want) <= 2 * T * (kmax + 4) * unit_roundoff(np.float32) * want)
  return got


@needs_lib
@pytest.mark.parametrize('W', WS)
def test_pagerank(sparse_ctx, W):
  sparse_ctx(W)
  from spartan_amd.examples.pagerank import site_graph
  n, k = 300, 6
  first = None
  for hint in (None, (50, n), (7, n)):
    Wm = site_graph(n, k, 0.9, seed=4, tile_hint=hint)
    G = Wm.glom()
    assert G.shape == (n, n) and G.dtype == np.float32
    assert np.allclose(np.asarray(G.sum(0)).ravel(), 1.0, atol=1e-6)  # column-normalised
    site = int(np.ceil(np.sqrt(n)))
    coo = G.tocoo()
    inside = (coo.row // site == coo.col // site)
    assert 0.8 < coo.data[inside].sum() / coo.data.sum() < 0.97  # same_site_prob = 0.9 (+ the random hits)
    if first is None:
      first = G
    _same_csr(G, first)  # the graph depends on the seed alone
    got = _check_pagerank(Wm, 5)
    assert abs(float(got.sum()) - 1.0) < 1e-4
  assert (site_graph(n, k, 0.9, seed=5).glom() != first).nnz > 0


@needs_lib
@pytest.mark.parametrize('W', WS)
def test_conj_gradient(sparse_ctx, W):
  sparse_ctx(W)
  from spartan_amd import expr
  from spartan_amd.examples.conj_gradient import cgit, conj_gradient
  n = 200
  A = _spd(n)
  d = A.diagonal()  # Gershgorin: every disc lies in [s / 2, 3 s / 2]
  radius = np.asarray(abs(A).sum(1)).ravel() - np.abs(d)
  assert (d - radius).min() >= d[0] / 2 - 1e-12 and (d + radius).max() <= 1.5 * d[0] + 1e-12
  x = np.random.RandomState(0).standard_normal((n, 1))
  for operand in (expr.from_numpy(A, tile_hint=(70, n)), A, expr.from_numpy(A.toarray(), tile_hint=(70, n))):
    z = cgit(operand, x).glom()
    assert z.shape == (n, 1) and z.dtype == np.float64
    # the CG bound 2 ((sqrt 3 - 1) / (sqrt 3 + 1))^15 sqrt 3 is about 1e-8: two decades left for rounding
    assert np.linalg.norm(A.dot(z) - x) / np.linalg.norm(x) <= 1e-6
  z = cgit(expr.from_numpy(A), np.zeros((n, 1))).glom()
  assert not z.any()
  v = conj_gradient(expr.from_numpy(A, tile_hint=(70, n)), num_iter=3).glom()
  assert v.shape == (n, 1) and abs(np.linalg.norm(v) - 1.0) <= 1e-12
  v32 = conj_gradient(expr.from_numpy(A.astype(np.float32)), num_iter=2).glom()
  assert v32.dtype == np.float32 and abs(np.linalg.norm(v32.astype(np.float64)) - 1.0) <= 1e-5
  nx = np.random.RandomState(1).standard_normal((50, 3))
  assert abs(float(expr.norm(expr.from_numpy(nx)).glom()) - np.linalg.norm(nx)) <= 1e-12 * np.linalg.norm(nx)


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
    from spartan_amd.examples.pagerank import site_graph
    from sparse_ref import SparseFakeBackend, assert_within, dense_data, same_bits, sparse_data
    backend.set_backend(SparseFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    ctx = runtime.get()
    assert ctx.world_size == world and ctx.dist_backend == 'gloo'
    for kind in ('ragged', 'skew', 'empty'):
      A = sparse_data(kind, M, N, np.float64)
      for hint in (None, (5, N), (1, N)):
        S = expr.from_numpy(A, tile_hint=hint)
        Sa = S.force()
        assert {ctx.owner(w) for w in Sa.tiles.values()} == {0, 1}  # both ranks own slabs
        assert set(Sa.local) == {e for e, w in Sa.tiles.items() if ctx.owner(w) == rank}
        _same_csr(S.glom(), A)
        assert Sa.nnz == A.nnz
        X = dense_data(N, 3, np.float64)
        for operand in (X, expr.from_numpy(X, tile_hint=(4, 3))):
          got = expr.dot(S, operand).glom()
          assert_within(got, A, X, np.zeros((M, 3)), 1.0, 0.0, 'gloo dot %s %s' % (kind, hint))
        assert same_bits(expr.todense(S).glom(), A.toarray())
        assert np.allclose(expr.sum(S).glom(), A.sum())
    # a matrix with fewer slabs than ranks own: rank 1 holds nothing and still takes part
    one = expr.from_numpy(sparse_data('uniform', M, N, np.float64), tile_hint=(M, N))
    assert {ctx.owner(w) for w in one.force().tiles.values()} == {0}
    assert expr.dot(one, np.ones(N)).glom().shape == (M,)
    _check_pagerank(site_graph(120, 5, 0.9, seed=2, tile_hint=(25, 120)), 4)
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
def test_world2_gloo_sparse(W):
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
def test_csrmm_plan_and_workspace():
  from spartan_amd import backend
  lib = _lib()
  for dt in (np.float32, np.float64):
    code = backend.spx_dtype(dt)
    for p in (1, 2, 3, 16, 64, 65, 1000):
      prev = 0
      T0 = None
      for mean in (0, 1, 2, 3, 7, 8, 9, 31, 33, 64, 100, 5000, 10 ** 6):
        for m in (1, 10, 1000, 10 ** 6):
          g, T, rpb = backend.csrmm_plan(dt, m, m * mean, p)
          assert 1 <= g <= 64 and g & (g - 1) == 0 and rpb * g == 256 and T >= 64
          T0 = T if T0 is None else T0
          assert T == T0  # one threshold for every problem: a row's chunks do not depend on the layout
        assert g >= prev  # non-decreasing in nnz / m
        prev = g
      assert backend.csrmm_plan(dt, 0, 0, p)[0] >= 1
    for p in (1, 16):
      last = -1
      for m, nnz in ((0, 0), (1, 0), (1, 1), (10, 100), (10, 10 ** 4), (1000, 10 ** 4), (1000, 10 ** 7),
                     (10 ** 6, 10 ** 7), (10 ** 6, 10 ** 9)):
        need = lib.spx_csrmm_workspace(code, m, nnz, p)
        assert need >= 0 and need >= last, (m, nnz, p, need, last)  # monotone in (m, nnz)
        assert lib.spx_csrmm_workspace(code, m, nnz, p + 7) >= need  # and in p
        # never more than a list entry and a partial row per chunk of T, and a list entry per long row
        _, T, _ = backend.csrmm_plan(dt, max(m, 1), nnz, p)
        chunks = nnz // T + min(m, nnz // (T + 1))
        assert need <= 64 + 24 * min(m, nnz // (T + 1)) + chunks * (16 + 8 * (p + 7))
        last = need
  with pytest.raises(TypeError):
    backend.csrmm_plan(np.int32, 4, 4, 1)
  with pytest.raises(ValueError):
    backend.csrmm_plan(np.float32, -1, 4, 1)
  assert lib.spx_csrmm_plan(99, 4, 4, 1, None, None, None) == -1 and lib.spx_csrmm_plan(1, 4, 4, 1, None, None, None) == -3
  assert lib.spx_csrmm_plan(3, 4, -1, 1, None, None, None) == -1 and lib.spx_csrmm_plan(3, 4, 4, 1, None, None, None) == 0
  for bad in ((99, 1, 1, 1), (1, 1, 1, 1), (3, -1, 1, 1), (3, 1, -1, 1), (3, 1, 1, -1)):
    assert lib.spx_csrmm_workspace(*bad) == -1, bad


@needs_lib
def test_argument_validation_without_gpu():
  """Every check of spx_csrmm / spx_csr_todense returns its code and message
  before any device work (there is no device here)."""
  lib = _lib()
  one = ctypes.c_void_p(64)  # a non-null pointer that is never followed: every call below fails validation

  def mm(dtype=3, m=4, n=4, p=2, nnz=8, rowptr=one, col=one, val=one, B=one, ldb=2, C=one, ldc=2, g=0, ws=None,
         ws_bytes=0):
    return lib.spx_csrmm(dtype, m, n, p, nnz, rowptr, col, val, B, ldb, C, ldc, 1.0, 0.0, g, ws, ws_bytes, 0, None)

  def err():
    return lib.spx_last_error()

  assert mm(dtype=99) == -1 and b'dtype' in err()
  assert mm(dtype=1) == -3 and b'float32 / float64' in err()
  for kw in ({'m': -1}, {'n': -1}, {'p': -1}, {'nnz': -1}):
    assert mm(**kw) == -1 and b'negative' in err(), kw
  assert mm(ldb=1) == -1 and b'leading dimension' in err()
  assert mm(ldc=1) == -1 and b'leading dimension' in err()
  for kw in ({'rowptr': None}, {'C': None}, {'col': None}, {'val': None}, {'B': None}):
    assert mm(**kw) == -1 and b'null' in err(), kw
  for g in (3, 128, -2):
    assert mm(g=g) == -1 and b'power of two' in err()
  big = 10 ** 5  # nnz above the long-row threshold: the workspace is needed
  assert mm(nnz=big) == -1 and b'workspace too small' in err()
  assert mm(nnz=big, ws=one, ws_bytes=8) == -1 and b'workspace too small' in err()
  # nothing to do: no pointer is looked at
  assert mm(m=0, rowptr=None, C=None) == 0 and mm(p=0, ldb=0, ldc=0, B=None, C=None) == 0

  def td(dtype=3, m=4, n=4, nnz=8, rowptr=one, col=one, val=one, D=one, ldd=4):
    return lib.spx_csr_todense(dtype, m, n, nnz, rowptr, col, val, D, ldd, None)

  assert td(dtype=99) == -1 and b'dtype' in err()
  assert td(dtype=2) == -3 and b'float32 / float64' in err()
  for kw in ({'m': -1}, {'n': -1}, {'nnz': -1}):
    assert td(**kw) == -1 and b'negative' in err(), kw
  assert td(ldd=3) == -1 and b'leading dimension' in err()
  for kw in ({'rowptr': None}, {'D': None}, {'col': None}, {'val': None}):
    assert td(**kw) == -1 and b'null' in err(), kw
  assert td(m=0, rowptr=None, D=None) == 0 and td(n=0, ldd=0) == 0


@needs_lib
def test_backend_wrappers_validate(sparse_ctx):
  """HipBackend.csrmm / csr_todense reject malformed tensors before the library sees them."""
  import torch
  from spartan_amd import backend
  be = backend.HipBackend.__new__(backend.HipBackend)  # no device: only the checks run
  rp = torch.zeros(5, dtype=torch.int64)
  col = torch.zeros(3, dtype=torch.int32)
  val = torch.zeros(3, dtype=torch.float32)
  B, C = torch.zeros(4, 2), torch.zeros(4, 2)
  for args in ((rp.to(torch.int32), col, val), (rp, col.to(torch.int64), val), (rp, col, val.to(torch.float16)),
               (rp, col, val[:2]), (rp.reshape(5, 1), col, val)):
    with pytest.raises(ValueError):
      be.csrmm(*args, 4, B, C)
    with pytest.raises(ValueError):
      be.csr_todense(*args, 4, torch.zeros(4, 4))
  for Bx, Cx in ((torch.zeros(5, 2), C), (B, torch.zeros(3, 2)), (B.double(), C), (B, torch.zeros(4, 3)),
                 (torch.zeros(2, 4).t(), C)):
    with pytest.raises(ValueError):
      be.csrmm(rp, col, val, 4, Bx, Cx)


def test_import_without_scipy():
  code = ('import sys; sys.modules["scipy"] = None; sys.path.insert(0, %r); import spartan_amd; '
          'from spartan_amd import expr; import spartan_amd.array.sparse, spartan_amd.expr.sparse; '
          'import spartan_amd.examples.conj_gradient; '
          'assert hasattr(expr, "sparse_rand") and "scipy.sparse" not in sys.modules; print("ok")' % ROOT)
  r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stderr[-2000:]

"""``sparse_transpose`` / ``SparseDistArray.transposed``, host logic (no GPU;
DESIGN.md 3.22): the glommed transpose against scipy bit for bit over source
layouts, target layouts and worker counts, the shape edge cases, the operations
the transpose opens (column sums, ``X @ S``), the refusals that stay, and two
gloo ranks.

The route runs here over the CPU test double (als_ref.AlsFakeBackend: NumPy
``sort`` / ``take`` / ``bincount`` / ``scan`` / ``csr_rowids``); the kernels it
calls are tested on the GPU in tests/test_sparse_transpose_gpu.py.
"""
import os
import socket
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, 'spartan_amd', 'libspx.so')

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')

M, N = 23, 17
HINTS = [None, (M, N), (5, N), (1, N), (4, N + 3)]
WS = [1, 3]


@pytest.fixture
def als_ctx(host_ctx):
  """host_ctx with the transpose- and ALS-capable test double installed."""
  from spartan_amd import backend
  from als_ref import AlsFakeBackend

  def make(num_workers=1):
    host_ctx(num_workers)
    be = AlsFakeBackend()
    backend.set_backend(be)
    return be
  return make


def scipy_transpose(A):
  W = A.T.tocsr()
  W.sort_indices()
  return W


def same_csr(got, want):
  import scipy.sparse as sp
  from sparse_ref import same_bits
  assert sp.isspmatrix_csr(got) and got.shape == want.shape and got.dtype == want.dtype
  assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
  assert got.indices.dtype == np.int32 and same_bits(got.data, want.data)


def tail_empty(dtype):
  """Data in the first 4 rows only: at one row per slab most slabs hold only empty rows."""
  import scipy.sparse as sp
  from sparse_ref import sparse_data
  return sp.vstack([sparse_data('uniform', 4, N, dtype, L=5), sp.csr_matrix((M - 4, N), dtype=dtype)]).tocsr()


def matrices(dtype):
  from sparse_ref import KINDS, sparse_data
  out = [(k, sparse_data(k, M, 1 if k == 'onecol' else N, dtype)) for k in KINDS]
  out.append(('tail_empty', tail_empty(dtype)))
  return out


def hint_for(hint, A):
  """``hint`` for a matrix of A's width (the 'onecol' kind has one column)."""
  return hint if hint is None else (hint[0], hint[1] - N + A.shape[1])


# ------------------------------------------------------------ round trip
@pytest.mark.parametrize('W', WS)
@pytest.mark.parametrize('hint', HINTS)
def test_transpose_equals_scipy(als_ctx, W, hint):
  als_ctx(W)
  from spartan_amd import expr
  from spartan_amd.array import sparse as sparray
  for dtype in (np.float32, np.float64):
    for kind, A in matrices(dtype):
      want = scipy_transpose(A)
      S = expr.from_numpy(A, tile_hint=hint_for(hint, A))
      T = expr.sparse_transpose(S)
      assert T.sparse_result and T.shape == want.shape and T.dtype == dtype
      Ta = T.force()
      assert isinstance(Ta, sparray.SparseDistArray) and Ta.tiles == sparray.slab_extents(want.shape)
      same_csr(T.glom(), want)
      # the array layer's method is the same route
      same_csr(S.force().transposed().glom(), want)
      for target in ((3, M), (1, M)):
        Tt = expr.sparse_transpose(S, tile_hint=target).force()
        assert Tt.tiles == sparray.slab_extents(want.shape, target)
        same_csr(Tt.glom(), want)
      # twice: A again, in any layout of the intermediate
      same_csr(expr.sparse_transpose(T).glom(), A)
      same_csr(expr.sparse_transpose(expr.sparse_transpose(S, tile_hint=(3, M)), tile_hint=(4, A.shape[1])).glom(), A)


@pytest.mark.parametrize('W', WS)
def test_transpose_shape_edge_cases(als_ctx, W):
  als_ctx(W)
  import scipy.sparse as sp
  from spartan_amd import expr
  from sparse_ref import sparse_data
  for dtype in (np.float32, np.float64):
    # explicit zeros survive, and every slab's count is filled
    A = sparse_data('uniform', M, N, dtype, L=6)
    A.data[::3] = 0
    assert A.nnz == M * 6 and (A.data == 0).sum() == M * 2
    for hint in HINTS:
      for target in (None, (3, M), (1, M)):
        Ta = expr.sparse_transpose(expr.from_numpy(A, tile_hint=hint), tile_hint=target).force()
        assert Ta.slab_nnz is not None and set(Ta.slab_nnz) == set(Ta.tiles)
        assert sum(Ta.slab_nnz.values()) == A.nnz == Ta.nnz
        got = Ta.glom()
        same_csr(got, scipy_transpose(A))
        assert got.nnz == A.nnz and (got.data == 0).sum() == M * 2
        for e, t in Ta.local.items():
          assert t.nnz == Ta.slab_nnz[e] and int(t.rowptr[0]) == 0 and int(t.rowptr[-1]) == t.nnz
          assert t.rowptr.numel() == e.shape[0] + 1
    # no entries at all, one row, one column
    for B in (sp.csr_matrix((M, N), dtype=dtype), sparse_data('uniform', 1, N, dtype, L=5),
              sparse_data('uniform', 1, N, dtype, L=N), sparse_data('onecol', M, 1, dtype),
              sp.csr_matrix(np.ones((M, 1), dtype)), sp.csr_matrix(np.ones((1, 1), dtype))):
      for hint in (None, (1, B.shape[1]), (4, B.shape[1])):
        T = expr.sparse_transpose(expr.from_numpy(B, tile_hint=hint))
        same_csr(T.glom(), scipy_transpose(B))
        same_csr(expr.sparse_transpose(T).glom(), B)


# ----------------------------------------------------- what it opens up
@needs_lib
@pytest.mark.parametrize('W', WS)
def test_column_sums_and_dense_times_sparse(als_ctx, W):
  als_ctx(W)
  from spartan_amd import expr
  from sparse_ref import assert_within, dense_data
  for dtype in (np.float32, np.float64):
    for kind, A in matrices(dtype):
      m, n = A.shape
      AT = scipy_transpose(A)
      for hint in (None, (5, n), (1, n)):
        T = expr.sparse_transpose(expr.from_numpy(A, tile_hint=hint))
        # column sums: a csrmm against ones, inside the summation bound
        got = expr.sum(T, axis=1).glom()
        assert got.shape == (n,) and got.dtype == dtype
        assert_within(got.reshape(n, 1), AT, np.ones((m, 1), dtype), np.zeros((n, 1), dtype), 1.0, 0.0,
                      'column sums %s %s' % (kind, hint))
        X = dense_data(m, 4, dtype)
        got = expr.dot(T, X).glom()
        assert_within(got, AT, X, np.zeros((n, 4), dtype), 1.0, 0.0, 'A.T @ X %s %s' % (kind, hint))
        # X @ S as transpose(dot(sparse_transpose(S), transpose(X)))
        Xr = dense_data(3, m, dtype, seed=2)
        got = expr.transpose(expr.dot(T, expr.transpose(expr.from_numpy(Xr)))).glom()
        assert got.shape == (3, n)
        assert_within(np.ascontiguousarray(got.T), AT, np.ascontiguousarray(Xr.T), np.zeros((n, 3), dtype), 1.0, 0.0,
                      'X @ A %s %s' % (kind, hint))


# ---------------------------------------------------------------- refusals
def test_bad_hint_and_the_refusals_that_stay(als_ctx):
  als_ctx(3)
  from spartan_amd import expr
  from sparse_ref import sparse_data
  A = sparse_data('uniform', M, N, np.float32)
  S = expr.from_numpy(A)
  for bad in ((3, M - 1), (N, 4), (1, 1)):
    with pytest.raises(NotImplementedError, match='row slabs'):
      expr.sparse_transpose(S, tile_hint=bad).force()
    with pytest.raises(NotImplementedError, match='row slabs'):
      S.force().transposed(tile_hint=bad)
  with pytest.raises(ValueError):
    expr.sparse_transpose(S, tile_hint=(3,)).force()
  with pytest.raises(TypeError):
    expr.sparse_transpose(A.toarray())
  # the transpose arrives under its own name only
  with pytest.raises(TypeError, match='todense'):
    S.T
  with pytest.raises(TypeError, match='todense'):
    expr.transpose(S)
  with pytest.raises(TypeError, match='todense'):
    expr.dot(np.ones((2, M), np.float32), S)
  with pytest.raises(NotImplementedError, match='transpose'):
    expr.sum(S, axis=0)
  with pytest.raises(TypeError, match='todense'):
    expr.sparse_transpose(S).T


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
    from als_ref import AlsFakeBackend
    from sparse_ref import sparse_data
    backend.set_backend(AlsFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    ctx = runtime.get()
    assert ctx.world_size == world and ctx.dist_backend == 'gloo'
    out = []
    for kind in ('ragged', 'skew', 'empty', 'banded'):
      A = sparse_data(kind, M, N, np.float64)
      A.data[::4] = 0  # explicit zeros travel too
      want = scipy_transpose(A)
      for hint in (None, (5, N), (1, N), (M, N)):
        S = expr.from_numpy(A, tile_hint=hint)
        for target in (None, (3, M), (1, M), (N, M)):
          Ta = expr.sparse_transpose(S, tile_hint=target).force()
          assert set(Ta.local) == {e for e, w in Ta.tiles.items() if ctx.owner(w) == rank}
          assert sum(Ta.slab_nnz.values()) == A.nnz
          got = Ta.glom()
          same_csr(got, want)
          out.append((got.indptr.tobytes(), got.indices.tobytes(), got.data.tobytes()))
        same_csr(expr.sparse_transpose(expr.sparse_transpose(S)).glom(), A)
    import hashlib
    h = hashlib.sha256()
    for parts in out:
      for b in parts:
        h.update(b)
    q.put((rank, 'ok ' + h.hexdigest()))
  except Exception:  # pragma: no cover - reported to the parent
    import traceback
    q.put((rank, traceback.format_exc()))
  finally:
    try:
      from spartan_amd import runtime
      runtime.shutdown()
    except Exception:
      pass


def run_two_ranks(body, W):
  """{rank: message} of ``body(rank, 2, port, W, queue)`` on two spawned gloo ranks."""
  import multiprocessing as mp
  ctx = mp.get_context('spawn')
  q = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=body, args=(r, 2, port, W, q)) for r in range(2)]
  for p in procs:
    p.start()
  res = {}
  for _ in procs:
    r, msg = q.get(timeout=240)
    res[r] = msg
  for p in procs:
    p.join(timeout=60)
  return res


@needs_lib
@pytest.mark.parametrize('W', [2, 3])
def test_world2_gloo_transpose(W):
  res = run_two_ranks(_gloo_body, W)
  for r in range(2):
    assert str(res.get(r)).startswith('ok '), res.get(r)
  assert res[0] == res[1]  # the glommed transposes are identical on both ranks

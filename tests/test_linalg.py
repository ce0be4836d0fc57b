"""``spartan_amd.cholesky`` / ``solve_triangular`` / ``cho_solve`` host logic (no
GPU): every route of the expression layer over tile layouts and worker counts,
laziness and validation, ``LinAlgError``, two gloo ranks, and the C-ABI
argument checks of spx_potrf / spx_trsm / spx_syrk.

The expression layer runs here over the CPU test double with scipy ``potrf`` /
``trsm`` / ``syrk`` (linalg_ref.LinalgFakeBackend); the kernels themselves are
tested on the GPU in tests/test_linalg_gpu.py.  Results are held to the derived
bounds of linalg_ref, not to a measured tolerance.
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

N = 50
# one tile, 2 x 2, 3 x 3, a ragged square grid, rows only, columns only, a non-square grid
HINTS = [(N, N), (25, 25), (17, 17), (20, 20), (13, N), (N, 21), (20, 13)]
GRIDS = {(25, 25), (17, 17), (20, 20)}


@pytest.fixture
def linalg_ctx(host_ctx):
  """host_ctx with the linalg-capable test double installed."""
  from spartan_amd import backend
  from linalg_ref import LinalgFakeBackend

  def make(num_workers=1):
    ctx = host_ctx(num_workers)
    be = LinalgFakeBackend()
    backend.set_backend(be)
    return be
  return make


def _replicated(a):
  import torch
  from spartan_amd import expr
  from spartan_amd.array import distarray
  return expr.lazify(distarray.ReplicatedArray(torch.as_tensor(a.copy())))


def _check_factor(A, got):
  from linalg_ref import assert_bound, potrf_ratio
  assert got.dtype == A.dtype and got.shape == A.shape
  assert not np.any(np.triu(got, 1)) and not np.any(np.signbit(np.triu(got, 1)))
  assert_bound(potrf_ratio(A, got), 'cholesky n=%d %s' % (A.shape[0], A.dtype))


# ------------------------------------------------------------- expr layer
@needs_lib
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_cholesky_every_route(linalg_ctx, W, dtype):
  be = linalg_ctx(W)
  from spartan_amd import expr
  from linalg_ref import spd_data
  for kind in ('wishart', 'illcond'):
    A = spd_data(kind, N, dtype, 1)
    dirty = A.copy()
    dirty[np.triu_indices(N, 1)] = np.nan  # only the lower triangle may be read
    for hint in HINTS:
      for src in (A, dirty):
        x = expr.from_numpy(src, tile_hint=hint).force()
        del be.calls[:]
        res = expr.cholesky(expr.lazify(x)).force()
        assert set(res.tiles) == set(x.tiles) and res.tiles == x.tiles, hint  # the input's tiling
        assert ('syrk' in be.calls) == (hint in GRIDS), (hint, be.calls)
        _check_factor(A, res.glom())
    _check_factor(A, expr.cholesky(_replicated(A)).glom())
    _check_factor(A, expr.cholesky(A).glom())  # a host array


@needs_lib
def test_cholesky_exact_kinds_and_tiny(linalg_ctx):
  linalg_ctx(3)
  from spartan_amd import expr
  from linalg_ref import exact_factor, same_bits, spd_data
  for dtype in (np.float32, np.float64):
    for kind in ('minij', 'diag'):
      for n, hint in ((1, None), (2, (1, 1)), (37, (10, 10)), (37, (37, 5))):
        A = spd_data(kind, n, dtype)
        got = expr.cholesky(expr.from_numpy(A, tile_hint=hint)).glom()
        assert same_bits(got, exact_factor(kind, n, dtype)), (kind, n, hint)


@needs_lib
def test_lazy_shape_dtype_and_composition(linalg_ctx):
  be = linalg_ctx(3)
  from spartan_amd import expr
  from spartan_amd.examples.cholesky import cholesky as example_cholesky
  r = np.random.RandomState(5)
  G = r.standard_normal((N, N))
  g = expr.from_numpy(G, tile_hint=(17, 17))
  gt = expr.from_numpy(np.ascontiguousarray(G.T), tile_hint=(17, 17))
  a = expr.dot(g, gt) * (1.0 / N) + expr.from_numpy(np.eye(N), tile_hint=(17, 17))
  del be.calls[:]
  e = example_cholesky(a)
  assert isinstance(e, expr.Expr) and e.shape == (N, N) and e.dtype == np.float64
  s = expr.solve_triangular(e, expr.ones((N, 3), dtype=np.float64))
  assert s.shape == (N, 3) and s.dtype == np.float64
  v = expr.cho_solve(e, expr.ones((N,), dtype=np.float64))
  assert v.shape == (N,) and v.dtype == np.float64
  assert 'potrf' not in be.calls and 'trsm' not in be.calls  # nothing ran yet
  A = a.glom()  # the factored matrix is the expression's own value, roundings included
  np.testing.assert_allclose(A, G.dot(G.T) / N + np.eye(N), rtol=1e-12)
  _check_factor(A, e.glom())
  # a map over the factor, and a reduction of it
  np.testing.assert_allclose((e * 2.0).glom(), 2.0 * np.linalg.cholesky(A), rtol=1e-10)
  np.testing.assert_allclose(expr.sum(e * e).glom(), np.trace(A), rtol=1e-12)
  np.testing.assert_allclose(v.glom(), np.linalg.solve(A, np.ones(N)), rtol=1e-10)


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_solve_triangular_routes(linalg_ctx, W, dtype):
  linalg_ctx(W)
  from spartan_amd import expr
  from linalg_ref import assert_bound, solve_ratio, spd_data
  L = np.linalg.cholesky(spd_data('wishart', N, np.float64, 2)).astype(dtype)
  r = np.random.RandomState(3)
  for bshape, bhints in (((N,), [None, (N,), (13,)]),
                         ((N, 7), [None, (N, 7), (N, 2), (13, 7), (20, 3)])):
    Bm = r.standard_normal(bshape).astype(dtype)
    for bh in bhints:
      for lh in ((N, N), (17, 17), (13, N)):
        for trans in (0, 1, 'N', 'T'):
          l = expr.from_numpy(L, tile_hint=lh)
          b = expr.from_numpy(Bm, tile_hint=bh).force()
          res = expr.solve_triangular(l, expr.lazify(b), trans=trans).force()
          assert res.tiles == b.tiles
          X = res.glom()
          assert X.shape == bshape and X.dtype == np.dtype(dtype)
          t = trans in (1, 'T')
          assert_bound(solve_ratio(L, X.reshape(N, -1), Bm.reshape(N, -1), 'L', t), 'solve %s %s %s' % (bh, lh, trans))
    X = expr.solve_triangular(_replicated(L), _replicated(Bm), trans=1).glom()
    assert_bound(solve_ratio(L, X, Bm, 'L', True), 'replicated solve')


@needs_lib
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_cho_solve_against_numpy(linalg_ctx, dtype):
  """(A + dA) x = b with |dA| <= gamma_{3n+1} |L| |L|^T (Higham, Theorem 10.4:
  the factorization's bound composed with the two solves'), so entrywise
  |A x - b| <= gamma_{3n+1} |L| |L|^T |x|, and against the fp64 solution of the
  same rounded system the normwise error is at most
  cond_inf(A) * gamma_{3n+1} * || |L| |L|^T ||_inf / ||A||_inf (to first order;
  doubled here for the second-order term and the reference's own error)."""
  linalg_ctx(3)
  from spartan_amd import expr
  from linalg_ref import LD, assert_bound, gamma, spd_data, _ratio
  A = spd_data('wishart', N, dtype, 4)
  Bm = np.random.RandomState(6).standard_normal((N, 4)).astype(dtype)
  a = expr.from_numpy(A, tile_hint=(20, 20))
  L = expr.cholesky(a)
  X = expr.cho_solve(L, expr.from_numpy(Bm, tile_hint=(13, 4))).glom()
  assert X.dtype == np.dtype(dtype) and X.shape == Bm.shape
  l = np.abs(L.glom().astype(LD))
  g = gamma(3 * N + 1, dtype)
  res = np.abs(A.astype(LD).dot(X.astype(LD)) - Bm.astype(LD))
  assert_bound(_ratio(res, g * l.dot(l.T).dot(np.abs(X.astype(LD)))), 'cho_solve residual')
  want = np.linalg.solve(A.astype(np.float64), Bm.astype(np.float64))
  a64 = A.astype(np.float64)
  tol = 2 * np.linalg.cond(a64, np.inf) * float(g) * float(np.abs(l.dot(l.T)).sum(1).max()) / np.abs(a64).sum(1).max()
  err = np.abs(X - want).max(0) / np.abs(want).max(0)
  print('cho_solve forward error %.3g, bound %.3g' % (err.max(), tol))
  assert err.max() <= tol


@needs_lib
def test_validation_errors(linalg_ctx):
  linalg_ctx(1)
  from spartan_amd import expr
  a = np.eye(4)
  with pytest.raises(ValueError, match='square'):
    expr.cholesky(np.ones((4, 5)))
  with pytest.raises(ValueError, match='square'):
    expr.cholesky(np.ones(4))
  with pytest.raises(TypeError, match='float32 / float64'):
    expr.cholesky(np.eye(4, dtype=np.int64))
  with pytest.raises(ValueError, match='trans'):
    expr.solve_triangular(a, np.ones(4), trans=2)
  with pytest.raises(ValueError, match='trans'):
    expr.solve_triangular(a, np.ones(4), trans='C')
  with pytest.raises(NotImplementedError, match='trans=1'):
    expr.solve_triangular(a, np.ones(4), lower=False)
  with pytest.raises(NotImplementedError, match='trans=0'):
    expr.solve_triangular(a, np.ones(4), trans='T', lower=False)
  with pytest.raises(ValueError, match='shape'):
    expr.solve_triangular(a, np.ones(5))
  with pytest.raises(ValueError, match='shape'):
    expr.solve_triangular(a, np.ones((4, 2, 2)))
  with pytest.raises(ValueError, match='square'):
    expr.solve_triangular(np.ones((4, 3)), np.ones(4))
  with pytest.raises(TypeError, match='mixed'):
    expr.solve_triangular(a, np.ones(4, np.float32))
  with pytest.raises(TypeError, match='float32 / float64'):
    expr.solve_triangular(np.eye(4, dtype=np.int32), np.ones(4, np.int32))


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_linalg_error_names_the_order(linalg_ctx, W):
  linalg_ctx(W)
  from spartan_amd import expr
  from linalg_ref import spd_data
  for dtype in (np.float32, np.float64):
    for j in (0, 16, 17, 33, N - 1):
      for bad in (-1.0, np.nan):
        A = spd_data('wishart', N, dtype, 9)
        A[j, j] = bad
        for hint in HINTS:
          with pytest.raises(np.linalg.LinAlgError, match=r'order %d is not' % (j + 1)):
            expr.cholesky(expr.from_numpy(A, tile_hint=hint)).force()
        with pytest.raises(np.linalg.LinAlgError, match=r'order %d is not' % (j + 1)):
          expr.cholesky(_replicated(A)).force()
    good = spd_data('wishart', N, dtype, 9)
    expr.cholesky(expr.from_numpy(good, tile_hint=(17, 17))).force()  # and a success afterwards


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
    from linalg_ref import LinalgFakeBackend, assert_bound, potrf_ratio, solve_ratio, spd_data
    backend.set_backend(LinalgFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    ctx = runtime.get()
    assert ctx.world_size == world and ctx.dist_backend == 'gloo'
    A = spd_data('wishart', N, np.float64, 1)
    Bm = np.random.RandomState(2).standard_normal((N, 5))
    bad = A.copy()
    bad[30, 30] = -1.0
    for hint in HINTS:
      x = expr.from_numpy(A, tile_hint=hint).force()
      if hint != (N, N):
        assert {ctx.owner(w) for w in x.tiles.values()} == {0, 1}
      res = expr.cholesky(expr.lazify(x)).force()
      assert res.tiles == x.tiles
      L = res.glom()
      assert not np.any(np.triu(L, 1))
      assert_bound(potrf_ratio(A, L), 'gloo cholesky %s' % (hint,))
      for bh in ((N, 2), (13, 5), None):
        for trans in (0, 1):
          X = expr.solve_triangular(expr.lazify(res), expr.from_numpy(Bm, tile_hint=bh), trans=trans).glom()
          assert_bound(solve_ratio(L, X, Bm, 'L', bool(trans)), 'gloo solve %s %s' % (hint, bh))
      try:
        expr.cholesky(expr.from_numpy(bad, tile_hint=hint)).force()
        raise AssertionError('no LinAlgError for %s' % (hint,))
      except np.linalg.LinAlgError as e:  # raised on every rank
        assert 'order 31 ' in str(e), str(e)
    v = expr.cho_solve(expr.cholesky(expr.from_numpy(A, tile_hint=(20, 20))), expr.from_numpy(Bm[:, 0], tile_hint=(13,)))
    np.testing.assert_allclose(v.glom(), np.linalg.solve(A, Bm[:, 0]), rtol=1e-10)
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
def test_world2_gloo_linalg(W):
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
def test_potrf_plan_and_workspace():
  from spartan_amd import backend
  lib = _lib()
  for dt in (np.float32, np.float64):
    nb, nbo = backend.potrf_plan(dt)
    assert 1 <= nb <= nbo and nbo % nb == 0
    assert lib.spx_potrf_workspace(backend.spx_dtype(dt), 0) == 0
    assert lib.spx_potrf_workspace(backend.spx_dtype(dt), 6400) >= 0
    for n, m in ((0, 5), (5, 0), (70, 3)):
      assert lib.spx_trsm_workspace(backend.spx_dtype(dt), 1, n, m) == 0  # RIGHT: kernels of their own
      assert lib.spx_trsm_workspace(backend.spx_dtype(dt), 0, n, m) == n * m * np.dtype(dt).itemsize
  with pytest.raises(TypeError):
    backend.potrf_plan(np.int32)
  assert lib.spx_potrf_plan(1, None, None) == -3 and lib.spx_potrf_plan(99, None, None) == -1
  for bad in ((1, 4), (99, 4), (3, -1), (3, 2 ** 31)):
    assert lib.spx_potrf_workspace(*bad) < 0, bad
  for bad in ((1, 0, 4, 4), (3, 2, 4, 4), (3, 0, -1, 4), (3, 1, 4, -1), (3, 0, 2 ** 31, 1)):
    assert lib.spx_trsm_workspace(*bad) < 0, bad


@needs_lib
def test_linalg_argument_validation_without_gpu():
  """Bad arguments are rejected before any device work (code + message).
  The pointers are host buffers: a call that got past its checks would try to
  launch on them, so every case here must stop at a check."""
  lib = _lib()
  bufs = [(ctypes.c_double * 64)() for _ in range(4)]
  a, l, c, info = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
  EINVAL, ENOTSUP = -1, -3
  err = lib.spx_last_error

  def potrf(dt, n, A=a, lda=None, L=l, ldl=None, inf=info, ws=None, nbytes=0):
    return lib.spx_potrf(dt, n, A, n if lda is None else lda, L, n if ldl is None else ldl, inf, ws, nbytes, None)

  assert potrf(99, 4) == EINVAL and b'dtype' in err()
  for dt in (0, 1, 2):
    assert potrf(dt, 4) == ENOTSUP and b'float32 / float64' in err()
  assert potrf(3, -1) == EINVAL and b'negative' in err()
  assert potrf(3, 4, inf=None) == EINVAL and b'null info' in err()
  assert potrf(3, 4, A=None) == EINVAL and b'null matrix' in err()
  assert potrf(4, 4, L=None) == EINVAL and b'null matrix' in err()
  assert potrf(3, 4, lda=3) == EINVAL and b'leading dimension' in err()
  assert potrf(4, 4, ldl=3) == EINVAL and b'leading dimension' in err()
  assert potrf(3, 4, L=a, lda=4, ldl=5) == EINVAL and b'in place' in err()
  assert potrf(3, 2 ** 31) == ENOTSUP and b'2^31' in err()
  assert potrf(3, 0, A=None, L=None, lda=0, ldl=0) == 0  # empty: no launch

  def trsm(dt, side, op, m, n, L=l, ldl=None, B=c, ldb=None, ws=a, nbytes=1 << 40):
    nl = m if side == 0 else n
    return lib.spx_trsm(dt, side, op, m, n, L, nl if ldl is None else ldl, B, n if ldb is None else ldb, ws, nbytes,
                        None)

  assert trsm(99, 0, 0, 4, 2) == EINVAL and b'dtype' in err()
  assert trsm(2, 0, 0, 4, 2) == ENOTSUP and b'float32 / float64' in err()
  assert trsm(3, 2, 0, 4, 2) == EINVAL and b'side' in err()
  assert trsm(3, 0, 2, 4, 2) == EINVAL and b'op' in err()
  assert trsm(3, 0, 0, -4, 2) == EINVAL and b'negative' in err()
  assert trsm(3, 1, 1, 4, -2) == EINVAL and b'negative' in err()
  assert trsm(3, 0, 0, 4, 2, L=None) == EINVAL and b'null matrix' in err()
  assert trsm(4, 1, 0, 4, 2, B=None) == EINVAL and b'null matrix' in err()
  assert trsm(3, 0, 0, 4, 2, ldl=3) == EINVAL and b'leading dimension' in err()
  assert trsm(3, 1, 0, 4, 2, ldl=1) == EINVAL and b'leading dimension' in err()
  assert trsm(3, 1, 1, 4, 2, ldb=1) == EINVAL and b'leading dimension' in err()
  for side in (0, 1):
    assert trsm(3, side, 0, 2 ** 31, 2 ** 31) == ENOTSUP and b'2^31' in err()
  need = lib.spx_trsm_workspace(4, 0, 4, 2)
  assert need == 64
  assert trsm(4, 0, 0, 4, 2, ws=None, nbytes=0) == EINVAL and b'workspace' in err()
  assert trsm(4, 0, 1, 4, 2, nbytes=need - 1) == EINVAL and b'workspace' in err()
  assert trsm(4, 0, 0, 4, 2, ws=None, nbytes=need) == EINVAL and b'workspace' in err()
  for m, n in ((0, 3), (3, 0), (0, 0)):
    for side in (0, 1):
      assert trsm(3, side, 0, m, n, ldl=4, ldb=4, ws=None, nbytes=0) == 0

  def syrk(dt, lower, M, N_, K, A=a, lda=None, B=l, ldb=None, C=c, ldc=None):
    return lib.spx_syrk(dt, lower, M, N_, K, A, K if lda is None else lda, B, K if ldb is None else ldb, C,
                        N_ if ldc is None else ldc, None)

  assert syrk(99, 0, 2, 2, 2) == EINVAL and b'dtype' in err()
  assert syrk(0, 0, 2, 2, 2) == ENOTSUP and b'float32 / float64' in err()
  for shape in ((-1, 2, 2), (2, -1, 2), (2, 2, -1)):
    assert syrk(3, 0, *shape) == EINVAL and b'negative' in err()
  assert syrk(3, 1, 3, 2, 2) == EINVAL and b'M == N' in err()
  for kw in (dict(A=None), dict(B=None), dict(C=None)):
    assert syrk(4, 0, 2, 2, 2, **kw) == EINVAL and b'null matrix' in err()
  for kw in (dict(lda=1), dict(ldb=1), dict(ldc=1)):
    assert syrk(3, 0, 2, 2, 2, **kw) == EINVAL and b'leading dimension' in err()
  assert syrk(3, 0, 2 ** 31, 2, 2) == ENOTSUP and b'2^31' in err()
  assert syrk(3, 1, 2 ** 30, 2 ** 30, 2) == ENOTSUP and b'2^31' in err()
  for shape in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
    assert syrk(3, 0, *shape) == 0

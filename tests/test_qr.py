"""``spartan_amd.qr`` host logic (no GPU): every route of the expression layer
over tile layouts and worker counts, laziness and validation, two gloo ranks,
the reference's qr / ssvd / pca tests, and the plan / workspace answers and
argument checks of spx_geqr / spx_orgqr.

The expression layer runs here over the CPU test double with scipy ``geqr`` /
``orgqr`` (qr_ref.QrFakeBackend); the kernels themselves are tested on the GPU
in tests/test_qr_gpu.py.  Results are held to the measured LAPACK yardsticks of
qr_ref.
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

M, N = 60, 10
# one tile; row slabs, several tiles per rank; row slabs whose last tile has fewer than N rows; column-cut tiles;
# two 2-d grids
HINTS = [(M, N), (7, N), (13, N), (M, 4), (20, 6), (13, 3)]


@pytest.fixture
def qr_ctx(host_ctx):
  """host_ctx with the qr-capable test double installed."""
  from spartan_amd import backend
  from qr_ref import QrFakeBackend

  def make(num_workers=1):
    host_ctx(num_workers)
    be = QrFakeBackend()
    backend.set_backend(be)
    return be
  return make


def _replicated(a):
  import torch
  from spartan_amd import expr
  from spartan_amd.array import distarray
  return expr.lazify(distarray.ReplicatedArray(torch.as_tensor(a.copy())))


def _check_pair(A, Q, R, what, ms=(M,)):
  from qr_ref import assert_ratios, check_r, yardstick
  assert Q.dtype == A.dtype and Q.shape == A.shape
  assert R.dtype == A.dtype and R.shape == (A.shape[1],) * 2
  check_r(R)
  assert_ratios(A, Q, R, yardstick(A.dtype, A.shape[1], ms), what)


# ------------------------------------------------------------- expr layer
@needs_lib
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_qr_every_route(qr_ctx, W, dtype):
  be = qr_ctx(W)
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from qr_ref import KINDS, qr_data
  for kind in KINDS:
    A = qr_data(kind, M, N, dtype)
    first = None
    for hint in HINTS:
      x = expr.from_numpy(A, tile_hint=hint).force()
      if hint == (13, N):
        assert min(e.shape[0] for e in x.tiles) < N
      if hint == (7, N) and W == 3:
        assert len(x.tiles) > 2 * W  # several tiles per worker
      del be.calls[:]
      qe, re_ = expr.qr(expr.lazify(x))
      q = qe.force()
      assert q.tiles == x.tiles, hint  # the input's tiling
      r = re_.force()
      assert isinstance(r, distarray.ReplicatedArray)
      Q, R = q.glom(), r.glom()
      _check_pair(A, Q, R, 'qr %s %s W=%d %s' % (kind, hint, W, np.dtype(dtype)))
      if kind == 'gauss':
        # full rank and well conditioned (cond_2 of a 60 x 10 Gaussian is below 3): the pair is unique, and R moves
        # by at most about cond * n * FACTOR * Y_res * u relative to its norm between routes (Higham, Theorem 19.6 /
        # Stewart's perturbation bound): below 1e3 u with room
        if first is None:
          first = R
        tol = 1e3 * (2.0 ** -24 if dtype == np.float32 else 2.0 ** -53)
        assert np.abs(R - first).max() <= tol * np.abs(first).max(), hint
    qe, re_ = expr.qr(_replicated(A))
    assert isinstance(qe.force(), distarray.ReplicatedArray) and isinstance(re_.force(), distarray.ReplicatedArray)
    _check_pair(A, qe.glom(), re_.glom(), 'qr %s replicated' % kind)
    qe, re_ = expr.qr(A)  # a host array
    _check_pair(A, qe.glom(), re_.glom(), 'qr %s host' % kind)


@needs_lib
def test_square_and_single_column(qr_ctx):
  qr_ctx(3)
  from spartan_amd import expr
  from qr_ref import qr_data
  for m, n, hint in ((9, 9, (4, 9)), (9, 9, (9, 9)), (31, 1, (5, 1)), (1, 1, None), (12, 5, (2, 5))):
    for dtype in (np.float32, np.float64):
      A = qr_data('gauss', m, n, dtype, 3)
      qe, re_ = expr.qr(expr.from_numpy(A, tile_hint=hint))
      _check_pair(A, qe.glom(), re_.glom(), 'qr %dx%d %s' % (m, n, hint), ms=(m,))


@needs_lib
def test_lazy_shape_dtype_and_one_factorization(qr_ctx):
  be = qr_ctx(3)
  from spartan_amd import expr
  from qr_ref import qr_data
  A = qr_data('gauss', M, N, np.float32, 5)
  x = expr.from_numpy(A, tile_hint=(13, N)).force()
  tiles = len(x.tiles)
  del be.calls[:]
  qe, re_ = expr.qr(expr.lazify(x))
  assert isinstance(qe, expr.Expr) and isinstance(re_, expr.Expr)
  assert qe.shape == (M, N) and re_.shape == (N, N) and qe.dtype == np.float32 and re_.dtype == np.float32
  prod = expr.dot(qe, re_)
  assert prod.shape == (M, N)
  assert 'geqr' not in be.calls and 'orgqr' not in be.calls  # nothing ran yet
  Q = qe.glom()
  tall = sum(1 for e in x.tiles if e.shape[0] >= N)
  assert tall == tiles - 1  # the last tile has fewer than N rows: its rows go on the stack as they are
  assert be.calls.count('geqr') == tall + 1  # once per tile, once for the stack
  R = re_.glom()
  assert be.calls.count('geqr') == tall + 1  # the pair shares one factorization
  _check_pair(A, Q, R, 'lazy pair')
  np.testing.assert_allclose(prod.glom(), A, atol=1e-5)
  np.testing.assert_allclose(expr.sum(qe * qe).glom(), N, rtol=1e-5)  # a map and a reduction over Q


@needs_lib
def test_validation_errors(qr_ctx):
  qr_ctx(1)
  from spartan_amd import backend, expr
  with pytest.raises(ValueError, match='2-d'):
    expr.qr(np.ones(4))
  with pytest.raises(ValueError, match='2-d'):
    expr.qr(np.ones((4, 2, 2)))
  with pytest.raises(TypeError, match='float32 / float64'):
    expr.qr(np.ones((4, 2), np.int64))
  with pytest.raises(NotImplementedError, match='tall or square'):
    expr.qr(np.ones((3, 4)))
  for dt in (np.float32, np.float64):
    nmax, _ = backend.geqr_plan(dt, 1)
    with pytest.raises(NotImplementedError, match='limit of %d' % nmax):
      expr.qr(np.ones((nmax + 5, nmax + 1), dt))
    expr.qr(np.ones((nmax, nmax), dt))  # the limit itself is accepted


# ------------------------------------------------- the reference's three tests
@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_reference_qr(qr_ctx, W):
  """tests/test_qr.py of the reference: randn 100 x 10 in tiles (25, 10)
  against scipy.linalg.qr, np.allclose of absolute values."""
  qr_ctx(W)
  from scipy import linalg
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from spartan_amd.examples.ssvd import qr
  Y = expr.randn(100, 10, tile_hint=(25, 10)).force()
  Q1, R1 = qr(Y)
  assert isinstance(Q1, distarray.DistArray) and isinstance(R1, np.ndarray)
  Q2, R2 = linalg.qr(Y.glom(), mode='economic')
  assert np.allclose(np.absolute(Q1.glom()), np.absolute(Q2))
  assert np.allclose(np.absolute(R1), np.absolute(R2))


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_reference_ssvd(qr_ctx, W):
  """tests/test_ssvd.py of the reference: randn 120 x 30 in row tiles of
  120 / W against np.linalg.svd."""
  qr_ctx(W)
  from spartan_amd import expr
  from spartan_amd.examples.ssvd import svd
  A = expr.randn(120, 30, tile_hint=(120 // W, 30), dtype=np.float64)
  U, S, VT = svd(A)
  U2, S2, VT2 = np.linalg.svd(A.glom(), full_matrices=0)
  assert np.allclose(np.absolute(U.glom()), np.absolute(U2))
  assert np.allclose(np.absolute(S), np.absolute(S2))
  assert np.allclose(np.absolute(VT), np.absolute(VT2))


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_reference_pca(qr_ctx, W):
  """tests/test_pca.py of the reference: PCA(10) on randn 40 x 20 against the
  top 10 right singular vectors of the centred data (what sklearn's PCA
  computes; sklearn is not assumed)."""
  qr_ctx(W)
  from spartan_amd import expr
  from spartan_amd.examples.pca import PCA
  data = np.random.RandomState(0).randn(40, 20)
  A = expr.from_numpy(data, tile_hint=(-(-40 // W), 20))
  m = PCA(10)
  m.fit(A)
  centred = data - data.mean(0)
  want = np.linalg.svd(centred, full_matrices=False)[2][:10]
  assert m.components_.shape == (10, 20)
  assert np.allclose(np.absolute(m.components_), np.absolute(want))
  low = m.transform(A)
  assert low.shape == (40, 10)
  np.testing.assert_allclose(np.absolute(low), np.absolute(centred.dot(want.T)), atol=1e-8)
  back = m.inverse_transform(low)
  np.testing.assert_allclose(back, centred.dot(want.T).dot(want) + data.mean(0), atol=1e-8)


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
    from spartan_amd.array import distarray
    from spartan_amd.config import FLAGS
    from qr_ref import QrFakeBackend, assert_ratios, check_r, qr_data, yardstick
    backend.set_backend(QrFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    ctx = runtime.get()
    assert ctx.world_size == world and ctx.dist_backend == 'gloo'
    for kind in ('gauss', 'illcond', 'rankdef'):
      A = qr_data(kind, M, N, np.float64, 1)
      yard = yardstick(np.float64, N, (M,), 1)
      for hint in HINTS:
        x = expr.from_numpy(A, tile_hint=hint).force()
        if hint != (M, N):
          assert {ctx.owner(w) for w in x.tiles.values()} == {0, 1}
        qe, re_ = expr.qr(expr.lazify(x))
        qa, ra = qe.force(), re_.force()
        assert qa.tiles == x.tiles and isinstance(ra, distarray.ReplicatedArray)
        R = ra.glom()  # this rank's own copy
        check_r(R)
        assert_ratios(A, qa.glom(), R, yard, 'gloo qr %s %s' % (kind, hint))
    from spartan_amd.examples.ssvd import svd
    Am = expr.randn(120, 30, tile_hint=(40, 30), dtype=np.float64)
    U, S, VT = svd(Am)
    U2, S2, VT2 = np.linalg.svd(Am.glom(), full_matrices=0)
    assert np.allclose(np.absolute(U.glom()), np.absolute(U2)) and np.allclose(S, S2)
    assert np.allclose(np.absolute(VT), np.absolute(VT2))
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
def test_world2_gloo_qr(W):
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
def test_geqr_plan_and_workspace():
  from spartan_amd import backend
  lib = _lib()
  for dt in (np.float32, np.float64):
    code = backend.spx_dtype(dt)
    size = np.dtype(dt).itemsize
    nmax, r1 = backend.geqr_plan(dt, 1)
    assert nmax >= 64
    for n in range(1, nmax + 1):
      lim, r = backend.geqr_plan(dt, n)
      assert lim == nmax and r >= 2 * n and r % 64 == 0
      # the block (n columns of r + 1), and its diagonal, fit the 160 KiB one workgroup may declare
      assert ((r + 1) * n + n) * size <= 160 * 1024
    assert backend.geqr_plan(dt, nmax + 1) == (nmax, 0)
    assert lib.spx_geqr_workspace(code, 0, 0) == 0 and lib.spx_geqr_workspace(code, 5, 0) == 0
    for n in (1, 17, nmax):
      _, r = backend.geqr_plan(dt, n)
      prev = 0
      for m in sorted({n, n + 1, r - 1, r, r + 1, 2 * r, 2 * r + 17, (r // n + 1) * r, (r // n + 1) * r + 1,
                       10 * r + 3, 1000 * r + 1, 2 ** 22}):
        if m < n:
          continue
        need = lib.spx_geqr_workspace(code, m, n)
        assert need >= prev and need % size == 0, (m, n, need, prev)  # monotone in m
        blocks = -(-m // r)
        assert need >= (blocks * r * n + blocks * n + n) * size  # the leaf reflectors, taus and the signs
        # every level at most halves-and-rounds-up the blocks (r >= 2 n): the reflectors of all levels are below
        # 2 blocks + one block per level, each level's stack is at most half its reflectors, 48 levels at the most
        # (and n taus per block)
        assert need <= ((3 * blocks + 100) * r * n + (2 * blocks + 100) * n) * size
        prev = need
  with pytest.raises(TypeError):
    backend.geqr_plan(np.int32, 4)
  assert lib.spx_geqr_plan(1, 4, None, None) == -3 and lib.spx_geqr_plan(99, 4, None, None) == -1
  assert lib.spx_geqr_plan(3, -1, None, None) == -1 and lib.spx_geqr_plan(3, 4, None, None) == 0
  for bad in ((1, 8, 4), (99, 8, 4), (3, -1, 0), (3, 4, -1), (3, 3, 4), (3, 1000, 129), (4, 1000, 65)):
    assert lib.spx_geqr_workspace(*bad) < 0, bad


@needs_lib
def test_qr_argument_validation_without_gpu():
  """Bad arguments are rejected before any device work (code + message).
  The pointers are host buffers: a call that got past its checks would try to
  launch on them, so every case here must stop at a check."""
  lib = _lib()
  bufs = [(ctypes.c_double * 64)() for _ in range(4)]
  a, r, w, c = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
  EINVAL, ENOTSUP = -1, -3
  err = lib.spx_last_error

  def geqr(dt, m, n, A=a, lda=None, R=r, ldr=None, ws=w, nbytes=1 << 40):
    return lib.spx_geqr(dt, m, n, A, n if lda is None else lda, R, n if ldr is None else ldr, ws, nbytes, None)

  assert geqr(99, 8, 4) == EINVAL and b'dtype' in err()
  for dt in (0, 1, 2):
    assert geqr(dt, 8, 4) == ENOTSUP and b'float32 / float64' in err()
  assert geqr(3, -1, 4) == EINVAL and b'negative' in err()
  assert geqr(3, 8, -4) == EINVAL and b'negative' in err()
  assert geqr(3, 3, 4) == EINVAL and b'tall or square' in err()
  assert geqr(3, 8, 4, A=None) == EINVAL and b'null matrix' in err()
  assert geqr(4, 8, 4, R=None) == EINVAL and b'null matrix' in err()
  assert geqr(3, 8, 4, lda=3) == EINVAL and b'leading dimension' in err()
  assert geqr(4, 8, 4, ldr=3) == EINVAL and b'leading dimension' in err()
  assert geqr(3, 1000, 129) == ENOTSUP and b'column limit 128' in err()
  assert geqr(4, 1000, 65) == ENOTSUP and b'column limit 64' in err()
  need = lib.spx_geqr_workspace(4, 8, 4)
  assert need > 0
  assert geqr(4, 8, 4, nbytes=need - 1) == EINVAL and b'workspace' in err()
  assert geqr(4, 8, 4, ws=None, nbytes=need) == EINVAL and b'workspace' in err()
  for m, n in ((0, 0), (5, 0)):
    assert geqr(3, m, n, A=None, R=None, ws=None, nbytes=0) == 0  # empty: no launch

  def orgqr(dt, m, n, ws=w, nbytes=1 << 40, C=c, ldc=None, Q=a, ldq=None):
    return lib.spx_orgqr(dt, m, n, ws, nbytes, C, n if ldc is None else ldc, Q, n if ldq is None else ldq, None)

  assert orgqr(99, 8, 4) == EINVAL and b'dtype' in err()
  assert orgqr(2, 8, 4) == ENOTSUP and b'float32 / float64' in err()
  assert orgqr(3, -8, 4) == EINVAL and b'negative' in err()
  assert orgqr(3, 3, 4) == EINVAL and b'tall or square' in err()
  assert orgqr(3, 8, 4, Q=None) == EINVAL and b'null matrix' in err()
  assert orgqr(3, 8, 4, ldq=3) == EINVAL and b'leading dimension' in err()
  assert orgqr(4, 8, 4, ldc=3) == EINVAL and b'leading dimension' in err()
  assert orgqr(3, 1000, 129) == ENOTSUP and b'column limit' in err()
  assert orgqr(4, 8, 4, nbytes=need - 1) == EINVAL and b'workspace' in err()
  assert orgqr(4, 8, 4, ws=None, nbytes=need) == EINVAL and b'workspace' in err()
  for m, n in ((0, 0), (5, 0)):
    assert orgqr(3, m, n, ws=None, nbytes=0, C=None, Q=None) == 0

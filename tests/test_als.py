"""``spartan_amd.examples.als`` and the boundary of spx_als_solve /
spx_csr_rowids, host logic (no GPU): the argument checks of
the library (they return before any device work), the driver over the CPU test
double (als_ref.AlsFakeBackend, whose ``als_solve`` is the float64 reference),
its refusals, and two gloo ranks.  The kernel itself is tested on the GPU in
tests/test_als_gpu.py.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from test_sparse_transpose import HERE, ROOT, als_ctx, needs_lib, run_two_ranks  # noqa: F401  (als_ctx: a fixture)


def rating_case(dtype=np.float64):
  """(A, R, mask): a 12 x 9 rating matrix of rank 2 with 60 % of its entries
  observed (scipy CSR), the full matrix and the observation mask."""
  import scipy.sparse as sp
  rs = np.random.RandomState(0)
  R = (rs.rand(12, 2).dot(rs.rand(2, 9)) + 0.5).astype(dtype)
  mask = np.zeros(12 * 9, bool)
  mask[rs.permutation(12 * 9)[:65]] = True  # 65 / 108 = 60 %
  mask = mask.reshape(12, 9)
  assert mask.any(0).all() and mask.any(1).all()  # every user and every item has a rating
  return sp.csr_matrix(np.where(mask, R, 0).astype(dtype)), R, mask


def rmse(U, M, R, mask):
  P = U.astype(np.float64).dot(M.astype(np.float64).T)
  return float(np.sqrt((((P - R) * mask) ** 2).sum() / mask.sum()))


# ------------------------------------------------------------ ABI, no GPU
@needs_lib
def test_als_plan():
  from spartan_amd import backend
  lib = backend.load_library()
  for dt in (np.float32, np.float64):
    for f in (1, 2, 20, 63, 64):
      assert backend.als_plan(dt, f) == (64, 4)
    for f in (0, 65, 1000):
      assert backend.als_plan(dt, f) == (64, 0)  # fmax whatever f is; no rows where f is outside 1 .. fmax
  with pytest.raises(TypeError):
    backend.als_plan(np.int32, 4)
  with pytest.raises(ValueError):
    backend.als_plan(np.float32, -1)
  assert lib.spx_als_plan(99, 4, None, None) == -1 and lib.spx_als_plan(1, 4, None, None) == -3
  assert lib.spx_als_plan(3, -1, None, None) == -1 and lib.spx_als_plan(3, 4, None, None) == 0  # outputs optional


@needs_lib
def test_argument_validation_without_gpu():
  """Every check of spx_als_solve / spx_csr_rowids returns its code and message
  before any device work (there is no device here)."""
  from spartan_amd import backend
  lib = backend.load_library()
  one, two = ctypes.c_void_p(64), ctypes.c_void_p(128)  # non-null, never followed: every call below fails validation

  def als(dtype=3, m=4, n=4, f=2, nnz=8, rowptr=one, col=one, val=one, Y=one, ldy=2, lam=0.5, X=two, ldx=2,
          info=one):
    return lib.spx_als_solve(dtype, m, n, f, nnz, rowptr, col, val, Y, ldy, lam, X, ldx, info, None)

  def err():
    return lib.spx_last_error()

  assert als(dtype=99) == -1 and b'dtype' in err()
  for dt in (0, 1, 2):
    assert als(dtype=dt) == -3 and b'float32 / float64' in err()
  for kw in ({'m': -1}, {'n': -1}, {'f': -1}, {'nnz': -1}):
    assert als(**kw) == -1 and b'negative' in err(), kw
  assert als(f=0, ldy=0, ldx=0) == -1 and b'below 1' in err()
  assert als(f=65, ldy=65, ldx=65) == -3 and b'fmax' in err()
  assert als(f=64, ldy=64, ldx=64, m=0) == 0
  assert als(n=2 ** 31) == -3 and b'int32' in err()
  assert als(ldy=1) == -1 and b'leading dimension' in err()
  assert als(ldx=1) == -1 and b'leading dimension' in err()
  for lam in (-0.5, float('inf'), float('nan')):
    assert als(lam=lam) == -1 and b'lambda' in err(), lam
  for kw in ({'rowptr': None}, {'X': None}, {'info': None}, {'col': None}, {'val': None}, {'Y': None}):
    assert als(**kw) == -1 and b'null' in err(), kw
  assert als(X=one) == -1 and b'alias' in err()
  # nothing to do: no pointer is looked at
  assert als(m=0, rowptr=None, X=None, info=None, col=None, val=None, Y=None) == 0

  def ids(m=4, nnz=8, rowptr=one, r0=0, out=one):
    return lib.spx_csr_rowids(m, nnz, rowptr, r0, out, None)

  for kw in ({'m': -1}, {'nnz': -1}, {'r0': -1}):
    assert ids(**kw) == -1 and b'negative' in err(), kw
  assert ids(r0=2 ** 31 - 4) == -3 and b'int32' in err()
  for kw in ({'rowptr': None}, {'out': None}):
    assert ids(**kw) == -1 and b'null' in err(), kw
  assert ids(m=0, rowptr=None, out=None) == 0 and ids(nnz=0, rowptr=None, out=None) == 0


@needs_lib
def test_backend_wrappers_validate():
  """HipBackend.als_solve / csr_rowids reject malformed tensors before the library runs anything."""
  import torch
  from spartan_amd import backend
  be = backend.HipBackend.__new__(backend.HipBackend)  # no device: only the checks run
  rp = torch.zeros(5, dtype=torch.int64)
  col = torch.zeros(3, dtype=torch.int32)
  val = torch.zeros(3, dtype=torch.float32)
  Y, X = torch.zeros(4, 2), torch.zeros(4, 2)
  for args in ((rp.to(torch.int32), col, val), (rp, col.to(torch.int64), val), (rp, col, val.to(torch.float16)),
               (rp, col, val[:2])):
    with pytest.raises(ValueError):
      be.als_solve(*args, 4, Y, 0.1, X)
  for Yx, Xx in ((torch.zeros(5, 2), X), (Y, torch.zeros(3, 2)), (Y.double(), X), (Y, torch.zeros(4, 3)),
                 (torch.zeros(2, 4).t(), X), (torch.zeros(4, 65), torch.zeros(4, 65)), (Y, Y)):
    with pytest.raises(ValueError):
      be.als_solve(rp, col, val, 4, Yx, 0.1, Xx)
  for lam in (-1.0, float('nan'), float('inf')):
    with pytest.raises(ValueError):
      be.als_solve(rp, col, val, 4, Y, lam, X)
  for rpx, out in ((rp.to(torch.int32), col), (rp, col.to(torch.int64)), (rp.reshape(5, 1), col)):
    with pytest.raises(ValueError):
      be.csr_rowids(rpx, 0, out)
  with pytest.raises(ValueError):
    be.csr_rowids(rp, 2 ** 31 - 3, col)


# ------------------------------------------------- driver, the test double
def _run_als(W, dtype, **kw):
  from spartan_amd.examples.als import als
  A, R, mask = rating_case(dtype)
  U, M = als(A, la=0.01, num_features=3, num_iter=kw.pop('num_iter', 15), seed=5, **kw)
  assert U.shape == (12, 3) and M.shape == (9, 3) and U.dtype == M.dtype == dtype
  return U.glom(), M.glom()


@needs_lib
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_als_reduces_the_error_and_ignores_the_layout(als_ctx, dtype):
  from als_ref import same_bits
  A, R, mask = rating_case(dtype)
  got = {}
  for W in (1, 3):
    be = als_ctx(W)
    from spartan_amd import expr
    from spartan_amd.examples.als import _initial_items, als
    from spartan_amd.array import sparse as sparray
    # the starting factors: random numbers, the items' average ratings in column 0
    M0 = _initial_items(sparray.transposed(sparray.from_scipy(A)), 3, 5).glom()
    assert M0.shape == (9, 3) and M0.dtype == dtype and (M0[:, 1:] >= 0).all() and (M0[:, 1:] < 1).all()
    avg = np.array([R[mask[:, j], j].astype(np.float64).mean() for j in range(9)])
    assert np.abs(M0[:, 0] - avg).max() <= 16 * float(np.finfo(dtype).eps) * avg.max()
    U0, _ = als(A, la=0.01, num_features=3, num_iter=1, M=M0, seed=5)
    before = rmse(U0.glom(), M0, R, mask)  # the initial M with the users solved against it
    del be.calls[:]
    U, M = _run_als(W, dtype)
    assert be.calls.count('als_solve') == 15 * 2 * W  # a launch per slab of A and of its transpose, per round
    after = rmse(U, M, R, mask)
    print('W %d %s: rmse on the observed entries %.4g -> %.4g' % (W, np.dtype(dtype), before, after))
    assert np.isfinite(after) and after < before
    # the same call again: the same bits (the seed fixes the start)
    U2, M2 = _run_als(W, dtype)
    assert same_bits(U, U2) and same_bits(M, M2)
    # a given M is the starting factor
    U3, M3 = _run_als(W, dtype, M=expr.from_numpy(M0, tile_hint=(4, 3)))
    assert same_bits(U, U3) and same_bits(M, M3)
    got[W] = (U, M)
  assert same_bits(got[1][0], got[3][0]) and same_bits(got[1][1], got[3][1])


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_half_step_matches_the_reference(als_ctx, W):
  als_ctx(W)
  import scipy.sparse as sp
  from spartan_amd import expr
  from spartan_amd.examples.als import half_step
  from als_ref import assert_within, factor_data, reference
  for dtype in (np.float32, np.float64):
    A, R, mask = rating_case(dtype)
    A = sp.vstack([A, sp.csr_matrix((2, 9), dtype=dtype)]).tocsr()  # two users without ratings
    A.data[3] = 0  # a stored zero is a missing rating
    Y = factor_data(9, 3, dtype)
    for hint in (None, (5, 9), (1, 9)):
      X, infos = half_step(expr.from_numpy(A, tile_hint=hint), Y, 0.01)
      Sa = expr.from_numpy(A, tile_hint=hint).force()
      Xa = X.force()
      assert {(e.ul[0], e.lr[0]): w for e, w in Xa.tiles.items()} == \
          {(e.ul[0], e.lr[0]): w for e, w in Sa.tiles.items()}
      assert all(e.shape[1] == 3 for e in Xa.tiles) and len(infos) == len(Sa.local)
      got = X.glom()
      assert got.dtype == dtype and not got[12:].any()
      assert_within(got, A, Y, 0.01, 'half step %s %s' % (np.dtype(dtype), hint))
    # the item side: the same solve over the transpose
    Ux = factor_data(14, 3, dtype, seed=1)
    X, _ = half_step(expr.sparse_transpose(expr.from_numpy(A)), Ux, 0.01)
    assert_within(X.glom(), A.T.tocsr(), Ux, 0.01, 'item half step %s' % np.dtype(dtype))


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_an_unrated_item_starts_at_zero(als_ctx, W):
  als_ctx(W)
  import scipy.sparse as sp
  from spartan_amd.array import sparse as sparray
  from spartan_amd.examples.als import _initial_items, als
  A, R, mask = rating_case()
  D = A.toarray()
  D[:, 4] = 0
  A = sp.csr_matrix(D)
  A[2, 4] = 0.0  # item 4: no rating, one stored zero
  A = A.tocsr()
  assert A.nnz == np.count_nonzero(D) + 1
  M0 = _initial_items(sparray.transposed(sparray.from_scipy(A)), 3, 7).glom()
  assert M0[4, 0] == 0 and np.isfinite(M0).all() and (M0[np.arange(9) != 4, 0] > 0).all()
  U, M = als(A, la=0.01, num_features=3, num_iter=2, seed=7)
  assert np.isfinite(U.glom()).all() and not M.glom()[4].any()  # nothing to fit: the item's factor is zero


@needs_lib
def test_refusals(als_ctx):
  als_ctx(3)
  from spartan_amd import expr
  from spartan_amd.examples.als import als
  A, R, mask = rating_case()
  with pytest.raises(TypeError, match='from_numpy'):
    als(A.toarray())
  with pytest.raises(TypeError, match='from_numpy'):
    als(expr.from_numpy(A.toarray()))
  with pytest.raises(NotImplementedError, match='implicit_feedback'):
    als(A, implicit_feedback=True)
  for la in (0, 0.0, -1.0, float('nan')):
    with pytest.raises(ValueError, match='la'):
      als(A, la=la)
  with pytest.raises(ValueError, match='64'):
    als(A, num_features=65)
  with pytest.raises(ValueError):
    als(A, num_features=0)
  with pytest.raises(ValueError):
    als(A, num_features=3, M=np.ones((9, 4)))
  with pytest.raises(ValueError):
    als(A, num_iter=0)


@needs_lib
def test_failed_rows_raise_once_at_the_end(als_ctx):
  """The counters of failed rows are read once, after the last iteration."""
  import torch
  be = als_ctx(3)
  from spartan_amd.examples.als import als
  A, R, mask = rating_case()
  solve = be.als_solve
  seen = []

  def failing(*a):
    solve(*a)
    seen.append(1)
    return torch.ones((1,), dtype=torch.int32) if len(seen) == 2 else torch.zeros((1,), dtype=torch.int32)
  be.als_solve = failing
  with pytest.raises(np.linalg.LinAlgError, match='1 row'):
    als(A, la=0.01, num_features=3, num_iter=2, seed=1)
  assert len(seen) == 2 * 2 * 3  # every half-step ran: nothing was read in between


# --------------------------------------------------------------- gloo ranks
def _gloo_body(rank, world, port, W, q):
  try:
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank), SPARTAN_SPMD_GUARD='strict',
                      SPARTAN_NCCL_TIMEOUT='240')
    from spartan_amd import backend, runtime
    from spartan_amd.config import FLAGS
    from als_ref import AlsFakeBackend
    backend.set_backend(AlsFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    assert runtime.get().world_size == world
    U, M = _run_als(W, np.float64, num_iter=4)
    q.put((rank, 'ok', U.tobytes(), M.tobytes()))
  except Exception:  # pragma: no cover - reported to the parent
    import traceback
    q.put((rank, traceback.format_exc(), b'', b''))
  finally:
    try:
      from spartan_amd import runtime
      runtime.shutdown()
    except Exception:
      pass


def _queue_adapter(rank, world, port, W, q):
  """``run_two_ranks`` reads (rank, message) pairs."""
  class Q:
    def put(self, item):
      q.put((item[0], item[1:]))
  _gloo_body(rank, world, port, W, Q())


@needs_lib
@pytest.mark.parametrize('W', [2, 3])
def test_world2_gloo_als(als_ctx, W):
  res = run_two_ranks(_queue_adapter, W)
  for r in range(2):
    assert res.get(r) is not None and res[r][0] == 'ok', res.get(r)
  assert res[0] == res[1]
  als_ctx(1)  # one rank, one worker: the same bits
  U, M = _run_als(1, np.float64, num_iter=4)
  assert res[0][1] == U.tobytes() and res[0][2] == M.tobytes()

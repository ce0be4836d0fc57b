"""spx_als_solve and the ALS driver on a real MI355X, at the
sizes where the kernel can go wrong: every register bucket of f and both ends
of the range, rows shorter than, equal to and longer than f, around the 64
lanes of a wave and well past them, and m around the four rows of a workgroup.

Results are compared with the float64 per-row reference of als_ref inside its
derived forward-error bound; reproducibility, independence of the neighbours
and the treatment of stored zeros are compared bit for bit.
"""
import numpy as np
import pytest

from als_ref import U64, assert_within, conditions, factor_data, reference, same_bits
from sparse_ref import _signed

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
FS = [1, 2, 3, 16, 20, 63, 64]
MS = [1, 3, 4, 5, 9]
PAD = 3


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _host(t):
  return np.ascontiguousarray(t.cpu().numpy())


def _csr_dev(A):
  return _dev(A.indptr.astype(np.int64)), _dev(A.indices.astype(np.int32)), _dev(A.data)


def _padded(a, fill=np.nan):
  """(buffer, view): ``a`` as the leading columns of a NaN-filled wider device buffer."""
  buf = np.full((a.shape[0], a.shape[1] + PAD), fill, a.dtype)
  buf[:, :a.shape[1]] = a
  t = _dev(buf)
  return t, t[:, :a.shape[1]]


def rows_csr(lengths, n, dtype, seed=0):
  """A (len(lengths), n) scipy CSR matrix whose row i stores lengths[i] entries
  with values in +-[0.5, 2): ascending columns drawn WITH repetition, so a row
  can be longer than n (the kernel walks stored entries; it never asks for
  distinct columns).  Nothing here is canonicalised."""
  import scipy.sparse as sp
  rs = np.random.RandomState(seed + 7919 * len(lengths) + 104729 * n + sum(lengths))
  indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
  indices = np.concatenate([np.sort(rs.randint(0, n, k)) for k in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
  A = sp.csr_matrix((_signed(rs, len(indices), dtype), indices, indptr), shape=(len(lengths), n))
  assert A.nnz == sum(lengths)
  return A


def _solve(be, A, Y, lam, csr=None):
  """(X, info) of one als_solve call on fresh device copies; X starts as NaN."""
  import torch
  from spartan_amd import backend
  csr = csr or _csr_dev(A)
  X = torch.full((A.shape[0], Y.shape[1]), float('nan'), dtype=backend.torch_dtype(Y.dtype), device='cuda')
  info = be.als_solve(csr[0], csr[1], csr[2], A.shape[1], _dev(Y), lam, X)
  return _host(X), int(info.item())


def _lengths(f):
  return [0, 1, max(f - 1, 0), f, 63, 64, 65, 257]


@pytest.mark.parametrize('f', FS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_als_solve_against_the_reference(gpu_ctx, dtype, f):
  from spartan_amd import backend
  be = backend.get()
  assert backend.als_plan(dtype, f) == (64, 4)
  L = _lengths(f)
  for n in (1, 40):
    Y = factor_data(n, f, dtype)
    for lam in (0.065, 1.0):
      for m in MS:
        for start in range(0, len(L), m):  # every length is used for every m
          lens = [L[(start + i) % len(L)] for i in range(m)]
          A = rows_csr(lens, n, dtype)
          what = 'f=%d n=%d lam=%g lens=%s %s' % (f, n, lam, lens, np.dtype(dtype))
          # the bound means something: every system is far from singular in the float64 working precision
          kap = conditions(A, Y, lam)
          assert kap.size == 0 or kap.max() < 1 / (1000 * U64), what
          X, info = _solve(be, A, Y, lam)
          assert info == 0, what
          assert_within(X, A, Y, lam, what)
          for i, k in enumerate(lens):
            if k == 0:
              assert not X[i].any(), what  # zeros, exactly


@pytest.mark.parametrize('dtype', DTYPES)
def test_stored_zeros_do_not_count(gpu_ctx, dtype):
  import scipy.sparse as sp
  from spartan_amd import backend
  be = backend.get()
  n = 40
  for f in (3, 20, 64):
    Y = factor_data(n, f, dtype)
    A = rows_csr([5, 70, 9, 1, 64, 2], n, dtype, seed=3)
    a, b = A.indptr[1], A.indptr[2]
    A.data[A.indptr[0]:A.indptr[1]] = 0       # row 0: stored zeros only
    A.data[a:b:3] = 0                         # row 1: zeros among the nonzeros, first entry included
    A.data[A.indptr[3]] = 0                   # row 3: its one entry is a zero
    A.data[A.indptr[5] - 1] = 0               # row 4: the last entry is a zero
    assert A.nnz == 151 and (A.data == 0).sum() == 5 + 24 + 1 + 1
    X, info = _solve(be, A, Y, 0.065)
    assert info == 0 and not X[0].any() and not X[3].any()
    # the same rows with the zeros removed: the same bits
    keep = A.data != 0
    lens = np.add.reduceat(keep.astype(np.int64), A.indptr[:-1])
    B = sp.csr_matrix((A.data[keep], A.indices[keep], np.concatenate([[0], np.cumsum(lens)])), shape=A.shape)
    assert B.nnz == 151 - 31 and np.diff(B.indptr).tolist() == [0, 46, 9, 0, 63, 2]
    X2, info2 = _solve(be, B, Y, 0.065)
    assert info2 == 0 and same_bits(X, X2)
    assert_within(X, A, Y, 0.065, 'stored zeros f=%d %s' % (f, np.dtype(dtype)))


@pytest.mark.parametrize('dtype', DTYPES)
def test_padding_reproducibility_independence(gpu_ctx, dtype):
  import torch
  from spartan_amd import backend
  be = backend.get()
  n = 40
  for f in (2, 20, 63):
    Y = factor_data(n, f, dtype)
    lens = [f, 0, 257, 1, 65, 64, 3, 63, max(f - 1, 0)]
    A = rows_csr(lens, n, dtype, seed=1)
    what = 'f=%d %s' % (f, np.dtype(dtype))
    X, info = _solve(be, A, Y, 0.065)
    assert info == 0
    # a second call: the same bits
    assert same_bits(_solve(be, A, Y, 0.065)[0], X), what
    # Y and X as the leading columns of NaN-filled wider buffers; nothing but X's leading columns is written
    csr = _csr_dev(A)
    keep = [t.clone() for t in csr]
    ybuf, yview = _padded(Y)
    xbuf, xview = _padded(np.full((len(lens), f), np.nan, dtype))
    ykeep = ybuf.clone()
    info = be.als_solve(csr[0], csr[1], csr[2], n, yview, 0.065, xview)
    assert int(info.item()) == 0 and same_bits(_host(xview), X), what
    assert np.isnan(_host(xbuf[:, f:])).all(), what
    assert torch.equal(ybuf[:, :f], ykeep[:, :f]) and np.isnan(_host(ybuf[:, f:])).all(), what
    for t, k in zip(csr, keep):
      assert torch.equal(t, k), what + ': the CSR arrays were written'
    # row i alone, as a one-row matrix: the same bits as inside the full matrix
    for i in range(len(lens)):
      one = A[i:i + 1].tocsr()
      assert one.nnz == lens[i]
      assert same_bits(_solve(be, one, Y, 0.065)[0], X[i:i + 1]), '%s row %d' % (what, i)


@pytest.mark.parametrize('dtype', DTYPES)
def test_failed_pivot(gpu_ctx, dtype):
  """lam = 0 and one entry: G = y y^T has rank 1 for f = 3.  With y = (2, 1, 4)
  every step is exact: G = [[4, 2, 8], [2, 1, 4], [8, 4, 16]], the first pivot
  is 4 and its root 2, the first column of L is (2, 1, 4), and the second pivot
  is 1 - 1 * 1 = 0.  The factorization stops at a pivot that is exactly zero: an
  arithmetic outcome.  The row is NaN and counted, and the rows around it are
  solved as usual."""
  import scipy.sparse as sp
  from spartan_amd import backend
  be = backend.get()
  n, f = 6, 3
  Y = factor_data(n, f, dtype)
  Y[0] = [2, 1, 4]
  # rows 1 and 4 hold one entry, column 0; the others hold 4 and 5 entries of independent factor rows
  rows = [[1, 2, 3, 4], [0], [1, 2, 3, 4, 5], [2, 3, 4, 5], [0], [1, 3, 4, 5]]
  indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
  indices = np.concatenate(rows).astype(np.int32)
  A = sp.csr_matrix((_signed(np.random.RandomState(2), len(indices), dtype), indices, indptr), shape=(6, n))
  good = [0, 2, 3, 5]
  assert conditions(A[good].tocsr(), Y, 0.0).max() < 1 / (1000 * U64)
  X, info = _solve(be, A, Y, 0.0)
  assert info == 2
  assert np.isnan(X[[1, 4]]).all() and np.isfinite(X[good]).all()
  assert_within(X[good], A[good].tocsr(), Y, 0.0, 'rows beside a failed one %s' % np.dtype(dtype))
  # the counter is cleared by every call
  X, info = _solve(be, A[good].tocsr(), Y, 0.0)
  assert info == 0 and np.isfinite(X).all()
  # with lam > 0 the same rows are solved
  X, info = _solve(be, A, Y, 0.5)
  assert info == 0
  assert_within(X, A, Y, 0.5, 'regularised %s' % np.dtype(dtype))


@pytest.mark.parametrize('dtype', DTYPES)
def test_driver(gpu_workers, dtype):
  from spartan_amd import expr
  from spartan_amd.array import sparse as sparray
  from spartan_amd.examples.als import _initial_items, als, half_step
  from test_als import rating_case, rmse
  A, R, mask = rating_case(dtype)
  got = {}
  for W in (1, 3):
    gpu_workers(W)
    U, M = als(A, la=0.01, num_features=3, num_iter=15, seed=5)
    assert U.shape == (12, 3) and M.shape == (9, 3) and U.dtype == M.dtype == dtype
    got[W] = (U.glom(), M.glom())
    M0 = _initial_items(sparray.transposed(sparray.from_scipy(A)), 3, 5).glom()
    # the first half-step: what the CPU double computes (the reference), inside the bound
    X, infos = half_step(expr.from_numpy(A), M0, 0.01)
    assert sum(int(i.item()) for i in infos) == 0
    X = X.glom()
    assert X.dtype == dtype
    assert_within(X, A, M0, 0.01, 'first half-step W=%d %s' % (W, np.dtype(dtype)))
    before = rmse(X, M0, R, mask)
    after = rmse(got[W][0], got[W][1], R, mask)
    print('W %d %s: rmse on the observed entries %.4g -> %.4g' % (W, np.dtype(dtype), before, after))
    assert after < before
  assert same_bits(got[1][0], got[3][0]) and same_bits(got[1][1], got[3][1])

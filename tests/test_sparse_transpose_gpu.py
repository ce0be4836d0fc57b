"""``sparse_transpose`` and spx_csr_rowids on a real MI355X, at
the sizes where the kernels behind the route can go wrong: around the longest
line spx_sort sorts in LDS, a column range that reaches the third radix digit,
one column shared by every entry (stability decides the order), and rows around
the 64 lanes of the wave that writes a row's ids.

Everything is compared with scipy bit for bit.
"""
import numpy as np
import pytest

from sparse_ref import sparse_data
from test_sparse_transpose import HINTS, M, N, hint_for, matrices, same_csr, scipy_transpose

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', DTYPES)
def test_small_matrices(gpu_workers, dtype, W):
  gpu_workers(W)
  from spartan_amd import expr
  for kind, A in matrices(dtype):
    want = scipy_transpose(A)
    for hint in HINTS:
      S = expr.from_numpy(A, tile_hint=hint_for(hint, A))
      for target in ((None, (3, M), (1, M)) if hint is None else (None,)):
        Ta = expr.sparse_transpose(S, tile_hint=target).force()
        assert sum(Ta.slab_nnz.values()) == A.nnz
        same_csr(Ta.glom(), want)
    same_csr(expr.sparse_transpose(expr.sparse_transpose(expr.from_numpy(A))).glom(), A)
  # explicit zeros survive
  A = sparse_data('uniform', M, N, dtype, L=6)
  A.data[::3] = 0
  got = expr.sparse_transpose(expr.from_numpy(A, tile_hint=(5, N))).glom()
  same_csr(got, scipy_transpose(A))
  assert (got.data == 0).sum() == M * 2


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nnz', [2047, 2048, 2049])
def test_around_the_lds_sort(gpu_workers, dtype, nnz):
  """One slab of 2047 / 2048 / 2049 entries: the LDS line sort and the first
  radix path of spx_sort; three slabs: the second, stable sort on the target.
  (300 rows of 6 or 7 entries, the explicit ``lengths`` of the 'ragged' kind --
  the kind of sparse_ref that takes a list of lengths.)"""
  from spartan_amd import backend, expr
  gpu_workers(1)
  m, n = 300, 40
  lengths = [nnz // m + (1 if i < nnz % m else 0) for i in range(m)]
  A = sparse_data('ragged', m, n, dtype, lengths=lengths)
  assert A.nnz == nnz
  assert backend.sort_plan(1, nnz, 1, np.int32, True)[0] == ('lds' if nnz <= backend.SORT_LDS_MAX else 'radix')
  want = scipy_transpose(A)
  same_csr(expr.sparse_transpose(expr.from_numpy(A, tile_hint=(m, n))).glom(), want)
  gpu_workers(3)
  same_csr(expr.sparse_transpose(expr.from_numpy(A, tile_hint=(100, n)), tile_hint=(7, m)).glom(), want)


@pytest.mark.parametrize('dtype', DTYPES)
def test_wide_matrix(gpu_workers, dtype):
  """70000 columns: the column keys differ in their third radix digit."""
  import scipy.sparse as sp
  gpu_workers(3)
  from spartan_amd import expr
  m, n, nnz = 50, 70000, 3000
  rs = np.random.RandomState(11)
  flat = np.sort(rs.choice(m * n, nnz, replace=False))
  A = sp.csr_matrix((rs.standard_normal(nnz).astype(dtype), (flat // n, flat % n)), shape=(m, n))
  A.sort_indices()
  assert A.nnz == nnz and A.indices.max() >= 1 << 16
  want = scipy_transpose(A)
  for hint, target in (((m, n), None), ((9, n), None), ((9, n), (4096, m))):
    same_csr(expr.sparse_transpose(expr.from_numpy(A, tile_hint=hint), tile_hint=target).glom(), want)


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_column(gpu_workers, dtype):
  """Every entry lands in the one row of the transpose: stability decides the order."""
  from spartan_amd import expr
  m = 5000  # 2500 entries: past the LDS sort
  A = sparse_data('onecol', m, 1, dtype)
  want = scipy_transpose(A)
  assert want.shape == (1, m) and np.array_equal(want.indices, np.arange(0, m, 2))
  for W, hint in ((1, (m, 1)), (3, None), (3, (700, 1))):
    gpu_workers(W)
    same_csr(expr.sparse_transpose(expr.from_numpy(A, tile_hint=hint)).glom(), want)


def test_csr_rowids(gpu_ctx):
  import torch
  from spartan_amd import backend
  be = backend.get()
  cases = [[0, 1, 63, 64, 65, 300], [300, 65, 64, 63, 1, 0], [7], [0], [300], [5, 0, 0, 0], [0, 0, 3, 0, 0],
           [1] * 9, [0] * 5, [64] * 4 + [0] * 3]
  for lens in cases:
    for r0 in (0, 17, 2 ** 31 - 1 - len(lens)):
      ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
      nnz = int(ip[-1])
      out = torch.full((nnz,), -7, dtype=torch.int32, device='cuda')
      rowptr = _dev(ip)
      keep = rowptr.clone()
      be.csr_rowids(rowptr, r0, out)
      want = np.repeat(np.arange(len(lens), dtype=np.int64) + r0, lens).astype(np.int32)
      assert np.array_equal(out.cpu().numpy(), want), (lens, r0)
      assert torch.equal(rowptr, keep)
  # the words behind the last entry are not touched
  buf = torch.full((40,), -7, dtype=torch.int32, device='cuda')
  be.csr_rowids(_dev(np.array([0, 10, 10, 30], np.int64)), 5, buf[:30])
  got = buf.cpu().numpy()
  assert np.array_equal(got[:30], np.repeat([5, 6, 7], [10, 0, 20])) and (got[30:] == -7).all()

"""Shared by tests/test_sparse.py and tests/test_sparse_gpu.py: the CPU test
double's ``csrmm`` / ``csr_todense`` (HipBackend's signatures, on scipy), the
data kinds, the exact-arithmetic case and the entrywise error bound of DESIGN.md
3.20.

The bound is Higham's for an inner product (Accuracy and Stability of Numerical
Algorithms, 2nd ed., eq. 3.5) and holds for EVERY summation order: row i of
C = alpha A B + beta C0 with k_i nonzeros is k_i products (one rounding each),
at most k_i - 1 additions on any path of any summation tree, the product with
alpha, the product beta C0 and the final addition -- at most k_i + 2 roundings
on any path:

    |C - exact|_ij <= gamma_{k_i + 2} (|alpha| (|A| |B|)_ij + |beta| |C0|_ij),
    gamma_k = k u / (1 - k u),

evaluated in np.longdouble.  It is a derived limit, not a measured tolerance.
"""
import numpy as np
import scipy.sparse as sp
import torch

from fake_backend import _np, _put
from linalg_ref import LD, _wide, same_bits, unit_roundoff  # noqa: F401  (re-exported)
from qr_ref import QrFakeBackend

KINDS = ('empty', 'diag', 'uniform', 'banded', 'skew', 'ragged', 'onecol')


def _rows_to_csr(cols_per_row, n, vals, dtype):
  lens = np.array([len(c) for c in cols_per_row], np.int64)
  indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  indices = np.concatenate([np.asarray(c, np.int64) for c in cols_per_row] + [np.zeros(0, np.int64)]).astype(np.int32)
  out = sp.csr_matrix((np.asarray(vals, dtype)[:len(indices)], indices, indptr), shape=(len(cols_per_row), n))
  out.has_sorted_indices = True
  return out


def structure(kind, m, n, rs, L=8, lengths=None):
  """Sorted, duplicate-free column lists, one per row.  kind:
    'empty'    no nonzeros;
    'diag'     the main diagonal;
    'uniform'  min(L, n) random columns in every row;
    'banded'   columns i - L//2 .. i + L//2 clipped to [0, n);
    'skew'     one row (the middle one) holds half of all nonzeros, the others
               alternate between empty and short (up to 3 entries);
    'ragged'   row lengths 0 .. L in shuffled order (or ``lengths``, shuffled);
    'onecol'   n = 1, every other row holds the one entry."""
  def pick(k):
    k = min(int(k), n)
    return np.sort(rs.choice(n, k, replace=False)) if k else np.zeros(0, np.int64)

  if kind == 'empty':
    return [np.zeros(0, np.int64) for _ in range(m)]
  if kind == 'diag':
    return [np.array([i], np.int64) if i < n else np.zeros(0, np.int64) for i in range(m)]
  if kind == 'uniform':
    return [pick(L) for _ in range(m)]
  if kind == 'banded':
    return [np.arange(max(0, i - L // 2), min(n, i + L // 2 + 1), dtype=np.int64) for i in range(m)]
  if kind == 'skew':
    rows = [pick(rs.randint(1, 4)) if i % 2 else np.zeros(0, np.int64) for i in range(m)]
    rest = sum(len(r) for r in rows)
    rows[m // 2] = pick(max(rest, 1))
    return rows
  if kind == 'ragged':
    lens = np.arange(m) % (L + 1) if lengths is None else np.resize(np.asarray(lengths), m)
    lens = rs.permutation(lens)
    return [pick(k) for k in lens]
  if kind == 'onecol':
    assert n == 1
    return [np.zeros(1, np.int64) if i % 2 == 0 else np.zeros(0, np.int64) for i in range(m)]
  raise ValueError(kind)


def _signed(rs, size, dtype):
  """Values in [0.5, 2) with random signs: nothing underflows or cancels to a denormal."""
  return ((0.5 + 1.5 * rs.random_sample(size)) * rs.choice([-1.0, 1.0], size)).astype(dtype)


def sparse_data(kind, m, n, dtype, seed=0, L=8, lengths=None):
  """An (m, n) scipy CSR matrix of ``dtype`` of the given kind with values in
  +-[0.5, 2)."""
  rs = np.random.RandomState(seed + 7919 * m + 104729 * n)
  rows = structure(kind, m, n, rs, L, lengths)
  nnz = sum(len(r) for r in rows)
  return _rows_to_csr(rows, n, _signed(rs, nnz, dtype), dtype)


def dense_data(n, p, dtype, seed=0):
  rs = np.random.RandomState(seed + 31 * n + p)
  return _signed(rs, (n, p), dtype)


def exact_case(kind, m, n, p, dtype, seed=0, L=8, lengths=None):
  """(A, B, C0) with small integer values: A in {-2 .. 2} \\ {0}, B and C0 in
  {-3 .. 3}.  A row has at most 2^16 nonzeros here (asserted), so every
  partial sum is below 2^16 * 6 < 2^24 in magnitude and exact in float32: any
  summation order gives the same bits.  (alpha and beta of the tests are
  multiples of 1/4 below 4, which keeps alpha acc + beta C0 exact too.)"""
  rs = np.random.RandomState(seed + 7919 * m + 104729 * n + p)
  rows = structure(kind, m, n, rs, L, lengths)
  assert max([len(r) for r in rows] + [0]) <= 2 ** 16
  nnz = sum(len(r) for r in rows)
  vals = rs.choice([-2.0, -1.0, 1.0, 2.0], nnz).astype(dtype)
  A = _rows_to_csr(rows, n, vals, dtype)
  B = rs.randint(-3, 4, (n, p)).astype(dtype)
  C0 = rs.randint(-3, 4, (m, p)).astype(dtype)
  return A, B, C0


def reference(A, B, C0, alpha, beta):
  """alpha A B + beta C0 by scipy in the data's dtype (beta == 0: C0 unread)."""
  dt = A.dtype
  r = dt.type(alpha) * np.asarray(A.dot(B), dtype=dt).reshape(A.shape[0], -1)
  if beta != 0:
    r = r + dt.type(beta) * C0
  return r.astype(dt)


def bound(A, B, C0, alpha, beta, u):
  """The entrywise Higham bound (m, p) in np.longdouble."""
  _wide(A.dtype)
  k = np.diff(A.indptr).astype(LD) + 2
  gam = (k * u / (1 - k * u))[:, None]
  absA = sp.csr_matrix((np.abs(A.data), A.indices, A.indptr), shape=A.shape)
  ab = exact(absA, np.abs(B), None, 1, 0)
  c0 = np.abs(C0).astype(LD) if beta != 0 else LD(0)
  return gam * (abs(LD(alpha)) * ab + abs(LD(beta)) * c0)


def exact(A, B, C0, alpha, beta):
  """alpha A B + beta C0 in np.longdouble (the products summed row by row)."""
  m = A.shape[0]
  Bl = B.astype(LD)
  out = np.zeros((m, B.shape[1]), LD)
  data = A.data.astype(LD)
  for i in range(m):
    a, b = A.indptr[i], A.indptr[i + 1]
    if b > a:
      out[i] = (data[a:b, None] * Bl[A.indices[a:b]]).sum(0)
  out = LD(alpha) * out
  if beta != 0:
    out = out + LD(beta) * C0.astype(LD)
  return out


def assert_within(C, A, B, C0, alpha, beta, what):
  u = unit_roundoff(A.dtype)
  err = np.abs(C.astype(LD) - exact(A, B, C0, alpha, beta))
  lim = bound(A, B, C0, alpha, beta, u)
  assert np.all(np.isfinite(C)), what
  worst = float((err / np.where(lim > 0, lim, 1)).max()) if err.size else 0.0
  print('%s: worst error / bound %.3g' % (what, worst))
  assert np.all(err <= lim), '%s: error %.4g of the bound' % (what, worst)


class SparseFakeBackend(QrFakeBackend):
  """QrFakeBackend + scipy ``csrmm`` / ``csr_todense``."""

  @staticmethod
  def _csr(rowptr, col, val, n):
    ip, c, v = _np(rowptr), _np(col), _np(val)
    assert ip.dtype == np.int64 and c.dtype == np.int32 and v.dtype in (np.float32, np.float64)
    assert ip.ndim == 1 and ip[0] == 0 and ip[-1] == len(c) == len(v)
    return sp.csr_matrix((v, c, ip), shape=(len(ip) - 1, int(n)))

  def csrmm(self, rowptr, col, val, n, B, C, alpha=1.0, beta=0.0, g=0, workspace=None):
    A = self._csr(rowptr, col, val, n)
    b, c0 = _np(B), _np(C)
    assert b.shape[0] == n and c0.shape == (A.shape[0], b.shape[1]) and b.dtype == A.dtype == c0.dtype
    assert g == 0 or (1 <= g <= 64 and g & (g - 1) == 0)
    _put(C, reference(A, b, c0, alpha, beta))
    self.calls.append('csrmm')

  def csr_todense(self, rowptr, col, val, n, D):
    A = self._csr(rowptr, col, val, n)
    assert tuple(D.shape) == A.shape and _np(D).dtype == A.dtype
    _put(D, A.toarray())
    self.calls.append('csr_todense')

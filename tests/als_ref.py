"""Shared by tests/test_als.py, tests/test_als_gpu.py and the sparse-transpose
tests: the per-row float64 reference of the ALS solve, its derived forward-error
bound and the CPU test double with ``als_solve`` /
``csr_rowids`` and everything the transpose route calls (``sort``, ``take``,
``bincount``, ``scan``, ``map``).

The solve.  For row i of the CSR matrix A with K_i = { k in the row : val[k] != 0 }
and k_i = |K_i|, Y_i the k_i x f matrix of the gathered rows y_{col[k]} and a_i
the k_i values:

    G_i = Y_i^T Y_i + lam k_i I,    b_i = Y_i^T a_i,    x_i = G_i^{-1} b_i.

The bound (``bound``), per row, with u = 2^-53 the unit roundoff of the float64
working precision of BOTH the kernel and the reference (float32 inputs convert
exactly) and gamma_j = j u / (1 - j u):

  1. Forming G_i and b_i.  An entry is a sum of k_i products (k_i roundings on
     the longest path of any summation order); the diagonal adds the rounded
     product lam k_i with one more addition.  So the computed G_i + dG1 and
     b_i + db have, entrywise,
         |dG1| <= gamma_{k_i + 1} (|Y_i|^T |Y_i| + lam k_i I),
         |db|  <= gamma_{k_i + 1} |Y_i|^T |a_i|.
  2. The Cholesky solve is backward stable (Higham, Accuracy and Stability of
     Numerical Algorithms, 2nd ed., Theorem 10.4): the computed x solves
     (G_i + dG1 + dG2) x = b_i + db with |dG2| <= gamma_{3 f + 1} |R^T| |R|, R the
     Cholesky factor.
  3. With eps_G = (|| |dG1| ||_2 + || |dG2| ||_2) / ||G_i||_2 and eps_b =
     || |db| ||_2 / ||b_i||_2 the normwise perturbation theorem (Higham, Theorem
     7.2) gives, for kappa = kappa_2(G_i) and kappa eps_G < 1,
         ||x^ - x_i||_2 <= kappa (eps_G + eps_b) / (1 - kappa eps_G) ||x_i||_2 =: E_i,
     and every entry of x^ - x_i is at most E_i in magnitude.
  4. The final rounding to the output dtype adds u_out |x^| <= u_out (|x_i| + E_i);
     u_out = 2^-24 for float32 and 0 for float64 (nothing is rounded again).

kappa, the norms and R are computed in float64 on the host from the reference
G_i.  ``reference`` itself is a float64 computation of the same kind -- the same
sums, then LAPACK's LU with partial pivoting, whose backward error gamma_{3 f}
|L| |U| is for a symmetric positive definite matrix (no pivot growth) of the size
of Cholesky's -- so it carries the error of steps 1 - 3 too.  What the tests
compare is the kernel against the reference, both within E_i of the exact x_i:

    |X - reference|_ij <= 2 E_i + u_out (|x_ij| + 2 E_i).

It is a derived limit, not a measured tolerance.
"""
import numpy as np
import scipy.sparse as sp
import torch

from fake_backend import _np, _put
from index_ref import IndexFakeBackend
from linalg_ref import LD, same_bits, unit_roundoff  # noqa: F401  (re-exported)
from scan_ref import ScanFakeBackend
from sparse_ref import SparseFakeBackend, _signed

U64 = float(2.0 ** -53)


def _gamma(j):
  assert j * U64 < 1
  return j * U64 / (1 - j * U64)


def _row(A, Y, i):
  """(Y_i, a_i) in float64: the gathered rows and the values of the entries of
  row i that are not zero."""
  a, b = A.indptr[i], A.indptr[i + 1]
  vals = A.data[a:b].astype(np.float64)
  keep = vals != 0
  return Y[A.indices[a:b][keep]].astype(np.float64), vals[keep]


def systems(A, Y, lam):
  """[(G_i, b_i) or None for an empty K_i] in float64."""
  A = sp.csr_matrix(A)
  out = []
  for i in range(A.shape[0]):
    Yi, ai = _row(A, Y, i)
    if len(ai) == 0:
      out.append(None)
      continue
    out.append((Yi.T.dot(Yi) + float(lam) * len(ai) * np.eye(Y.shape[1]), Yi.T.dot(ai)))
  return out


def reference(A, Y, lam):
  """The (m, f) float64 solution, row by row: np.linalg.solve of the definition
  (it raises on a singular system); a row without nonzero entries gives zeros."""
  sys_ = systems(A, Y, lam)
  X = np.zeros((len(sys_), Y.shape[1]), np.float64)
  for i, gb in enumerate(sys_):
    if gb is not None:
      X[i] = np.linalg.solve(gb[0], gb[1])
  return X


def conditions(A, Y, lam):
  """kappa_2(G_i) of every row with a system (float64)."""
  return np.array([np.linalg.cond(gb[0], 2) for gb in systems(A, Y, lam) if gb is not None])


def bound(A, Y, lam, u):
  """The (m, f) entrywise limit of |X - reference(A, Y, lam)| derived in the
  module docstring; ``u`` is the unit roundoff of the output dtype."""
  A = sp.csr_matrix(A)
  f = Y.shape[1]
  u_out = float(u) if float(u) > 2 * U64 else 0.0
  X = reference(A, Y, lam)
  out = np.zeros(X.shape, np.float64)
  for i, gb in enumerate(systems(A, Y, lam)):
    if gb is None:
      continue  # zeros, exactly
    G, b = gb
    Yi, ai = _row(A, Y, i)
    k = len(ai)
    absG = np.abs(Yi).T.dot(np.abs(Yi)) + float(lam) * k * np.eye(f)
    absb = np.abs(Yi).T.dot(np.abs(ai))
    R = np.linalg.cholesky(G).T
    nG = np.linalg.norm(G, 2)
    eps_G = (_gamma(k + 1) * np.linalg.norm(absG, 2) + _gamma(3 * f + 1) * np.linalg.norm(np.abs(R.T).dot(np.abs(R)), 2)) / nG
    nb = np.linalg.norm(b)
    eps_b = _gamma(k + 1) * np.linalg.norm(absb) / nb if nb > 0 else 0.0
    kappa = np.linalg.cond(G, 2)
    assert kappa * eps_G < 1, 'row %d: kappa %.3g is too large for the bound to mean anything' % (i, kappa)
    E = kappa * (eps_G + eps_b) / (1 - kappa * eps_G) * np.linalg.norm(X[i])
    out[i] = 2 * E + u_out * (np.abs(X[i]) + 2 * E)
  return out


def assert_within(X, A, Y, lam, what, rows=None):
  """|X - reference| <= bound entrywise (``rows``: only those rows of A)."""
  u = unit_roundoff(X.dtype)
  ref, lim = reference(A, Y, lam), bound(A, Y, lam, u)
  if rows is not None:
    ref, lim = ref[rows], lim[rows]
  assert X.shape == ref.shape and np.all(np.isfinite(X)), what
  err = np.abs(X.astype(np.float64) - ref)
  worst = float((err / np.where(lim > 0, lim, 1)).max()) if err.size else 0.0
  print('%s: worst error / bound %.3g' % (what, worst))
  assert np.all(err <= lim), '%s: error %.4g of the bound' % (what, worst)


def factor_data(n, f, dtype, seed=0):
  """An (n, f) factor with entries in +-[0.5, 2)."""
  return _signed(np.random.RandomState(seed + 131 * n + f), (n, f), dtype)


class AlsFakeBackend(SparseFakeBackend, IndexFakeBackend, ScanFakeBackend):
  """SparseFakeBackend + NumPy ``take`` / ``scan`` and the CPU ``als_solve`` /
  ``csr_rowids`` (HipBackend's signatures)."""

  def csr_rowids(self, rowptr, r0, out):
    ip = _np(rowptr)
    assert ip.dtype == np.int64 and ip.ndim == 1 and ip[0] == 0 and ip[-1] == out.numel()
    assert _np(out).dtype == np.int32 and out.dim() == 1
    if out.numel():
      _put(out, np.repeat(np.arange(len(ip) - 1, dtype=np.int64) + int(r0), np.diff(ip)).astype(np.int32))
    self.calls.append('csr_rowids')

  def als_solve(self, rowptr, col, val, n, Y, lam, X):
    A = self._csr(rowptr, col, val, n)
    y = _np(Y)
    assert y.shape[0] == n and tuple(X.shape) == (A.shape[0], y.shape[1]) and y.dtype == A.dtype == _np(X).dtype
    assert lam >= 0
    if A.shape[0]:
      _put(X, reference(A, y, lam).astype(A.dtype))
    self.calls.append('als_solve')
    return torch.zeros((1,), dtype=torch.int32)

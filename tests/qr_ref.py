"""Shared by tests/test_qr.py and tests/test_qr_gpu.py: the CPU test double's
``geqr`` / ``orgqr`` (HipBackend's signatures, on scipy's LAPACK), the data
kinds and the two error ratios of DESIGN.md 3.19.

With u the unit roundoff of the data's dtype, evaluated in np.longdouble:

  res  = max_j ||a_j - Q r_j||_2 / (u ||a_j||_2)   over the nonzero columns (a
         zero column must give an exactly zero residual),
  orth = ||Q^T Q - I||_2 / u.

Higham (Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 19.4)
bounds both by a gamma~_{mn} whose constant the theory leaves open, so the
bound is not derived here: it is MEASURED against the reference implementation.
For every (dtype, n) the yardsticks Y_res and Y_orth are the largest ratios
that LAPACK's Householder QR (``scipy.linalg.qr(mode='economic')`` in the
data's dtype) gives over all data kinds and all m of the test's list at that
n; a result passes when each of its ratios is at most FACTOR = 4 times its
yardstick.  The 4 is the allowance for a different but equally valid order of
reflectors and sums (tree versus column-sequential, FMA chains): a blockwise
TSQR built from LAPACK blocks stays within 2.2 x the same-input LAPACK ratio
over these kinds (m <= 20000, n <= 64, LAPACK ratios of 1-18 u).
"""
import numpy as np
import torch

from fake_backend import _np, _put
from linalg_ref import LD, LinalgFakeBackend, _wide, same_bits, unit_roundoff  # noqa: F401  (re-exported)

KINDS = ('gauss', 'illcond', 'graded', 'rankdef')
FACTOR = 4


def qr_data(kind, m, n, dtype, seed=0):
  """An (m, n) matrix of ``dtype``, m >= n.  kind:
    'gauss'    standard normal;
    'illcond'  U diag(logspace(0, -6 | -14)) V^T (float32 | float64), U and V
               with orthonormal columns: the case CholeskyQR cannot do;
    'graded'   Gaussian columns scaled by logspace(0, 15 | 100);
    'rankdef'  the right half repeats the left half, and column 2 is zero."""
  dt = np.dtype(dtype)
  f32 = dt == np.float32
  r = np.random.RandomState(seed + 7919 * m + 104729 * n)
  G = r.standard_normal((m, n))
  if kind == 'gauss':
    A = G
  elif kind == 'illcond':
    U, _ = np.linalg.qr(G)
    V, _ = np.linalg.qr(r.standard_normal((n, n)))
    A = (U * np.logspace(0, -6 if f32 else -14, n)).dot(V.T)
  elif kind == 'graded':
    A = G * np.logspace(0, 15 if f32 else 100, n)
  elif kind == 'rankdef':
    A = G.copy()
    h = n // 2
    if n > 2:
      A[:, 2] = 0.0
    if h:
      A[:, n - h:] = A[:, :h]
  else:
    raise ValueError(kind)
  return np.ascontiguousarray(A.astype(dt))


def qr_ratios(A, Q, R):
  """(res, orth) of the factorization Q R of A, in units of u."""
  dt = A.dtype
  _wide(dt)
  m, n = A.shape
  assert Q.shape == (m, n) and R.shape == (n, n) and Q.dtype == dt and R.dtype == dt
  assert np.all(np.isfinite(Q)) and np.all(np.isfinite(R)), 'non-finite entries in the factors'
  u = unit_roundoff(dt)
  a, q, r = A.astype(LD), Q.astype(LD), R.astype(LD)
  d = a - q.dot(r)
  rn = np.sqrt((d * d).sum(0))
  an = np.sqrt((a * a).sum(0))
  zero = an == 0
  assert not np.any(rn[zero] != 0), 'a nonzero residual in a zero column'
  res = float(np.max(rn[~zero] / (u * an[~zero]))) if np.any(~zero) else 0.0
  e = q.T.dot(q) - np.eye(n, dtype=LD)
  scale = np.abs(e).max()
  orth = 0.0
  if scale > 0:  # the 2-norm of the scaled matrix in double: 1e-16 relative, on a quantity of a few u
    orth = float(LD(np.linalg.norm((e / scale).astype(np.float64), 2)) * scale / u)
  return res, orth


def lapack_qr(A):
  from scipy.linalg import qr
  if A.shape[1] == 0:
    return np.zeros(A.shape, A.dtype), np.zeros((0, 0), A.dtype)
  Q, R = qr(A, mode='economic', check_finite=False)
  return Q.astype(A.dtype), np.triu(R).astype(A.dtype)


_YARD = {}


def yardstick(dtype, n, ms, seed=0):
  """(Y_res, Y_orth): LAPACK's largest ratios over KINDS and ``ms`` at n."""
  key = (np.dtype(dtype).str, n, tuple(ms), seed)
  if key not in _YARD:
    yr = yo = 0.0
    for kind in KINDS:
      for m in ms:
        A = qr_data(kind, m, n, dtype, seed)
        res, orth = qr_ratios(A, *lapack_qr(A))
        yr, yo = max(yr, res), max(yo, orth)
    _YARD[key] = (yr, yo)
  return _YARD[key]


def assert_ratios(A, Q, R, yard, what):
  """Both ratios within FACTOR x the yardstick; returns them."""
  res, orth = qr_ratios(A, Q, R)
  print('%s: res %.3g u (yardstick %.3g), orth %.3g u (yardstick %.3g)' % (what, res, yard[0], orth, yard[1]))
  assert res <= FACTOR * yard[0], '%s: residual %.4g u against %d x %.4g u' % (what, res, FACTOR, yard[0])
  assert orth <= FACTOR * yard[1], '%s: orthogonality %.4g u against %d x %.4g u' % (what, orth, FACTOR, yard[1])
  return res, orth


def check_r(R, bits=False):
  """Upper triangular with a non-negative diagonal; ``bits``: the strict lower
  triangle is +0.0 bit for bit."""
  n = R.shape[0]
  low = np.tril_indices(n, -1)
  assert not np.any(R[low])
  if bits:
    assert not np.any(np.ascontiguousarray(R).view({4: np.uint32, 8: np.uint64}[R.dtype.itemsize])[low])
  assert np.all(np.diag(R) >= 0)


class _FakeQr:
  def __init__(self, q):
    self.q = q


class QrFakeBackend(LinalgFakeBackend):
  """LinalgFakeBackend + scipy ``geqr`` / ``orgqr``: the handle holds the
  economic Q, and ``orgqr`` is Q_econ @ C."""

  def geqr(self, A):
    a = _np(A)
    assert a.ndim == 2 and a.shape[0] >= a.shape[1] and a.dtype in (np.float32, np.float64)
    q, r = lapack_qr(a)
    self.calls.append('geqr')
    return torch.as_tensor(np.ascontiguousarray(r)), _FakeQr(q)

  def orgqr(self, handle, C, Q):
    assert isinstance(handle, _FakeQr)
    q = handle.q
    assert tuple(Q.shape) == q.shape and _np(Q).dtype == q.dtype
    if C is not None:
      c = _np(C)
      assert c.shape == (q.shape[1],) * 2 and c.dtype == q.dtype
      q = q.dot(c)
    _put(Q, q)
    self.calls.append('orgqr')

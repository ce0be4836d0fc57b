"""Shared by tests/test_linalg.py and tests/test_linalg_gpu.py: the CPU test
double's ``potrf`` / ``trsm`` / ``syrk`` (HipBackend's signatures, on scipy's
LAPACK), the data kinds and the derived error bounds of DESIGN.md 3.18.

The bounds are Higham's (Accuracy and Stability of Numerical Algorithms, 2nd
ed., Theorems 10.3 and 8.5): with u the unit roundoff of the data's dtype and
gamma_k = k u / (1 - k u),

  |A - L L^T| <= gamma_{n+1} |L| |L|^T      on the lower triangle,
  |op(L) X - B| <= gamma_n |L| |X|           for each solve,
  |C0 - A B^T - C| <= gamma_{K+1} (|C0| + |A| |B|^T)   for the update,

entrywise, for any order of the sums (FMA chains, blocked and tiled forms
alike).  Residuals and bounds are evaluated in np.longdouble, which must be
wider than the data.
"""
import numpy as np
import torch

from spartan_amd import backend as B
from fake_backend import _np, _put
from topk_ref import TopkFakeBackend, same_bits  # noqa: F401  (same_bits: re-exported)

LD = np.longdouble
KINDS = ('wishart', 'illcond', 'minij', 'diag')


def unit_roundoff(dtype):
  return LD(2) ** -24 if np.dtype(dtype) == np.float32 else LD(2) ** -53


def gamma(k, dtype):
  u = unit_roundoff(dtype)
  assert k * u < 1
  return k * u / (1 - k * u)


def _wide(dtype):
  """np.longdouble must carry more mantissa bits than the data."""
  assert np.finfo(LD).nmant > np.finfo(np.dtype(dtype)).nmant, \
      'np.longdouble (%d mantissa bits) is not wider than %s' % (np.finfo(LD).nmant, np.dtype(dtype))
  if np.dtype(dtype) == np.float64:
    assert np.finfo(LD).nmant >= 63


def spd_data(kind, n, dtype, seed=0):
  """A symmetric positive definite (n, n) matrix of ``dtype``.  kind:
    'wishart'  G G^T / n + I, G standard normal;
    'illcond'  Q diag(logspace(0, -4 | -10)) Q^T (float32 | float64), Q
               orthogonal, symmetrised after rounding;
    'minij'    A[i, j] = min(i, j) + 1: the factor is exactly tril(ones);
    'diag'     squares of small integers on the diagonal."""
  dt = np.dtype(dtype)
  r = np.random.RandomState(seed + 7919 * n)
  if kind == 'wishart':
    G = r.standard_normal((n, n))
    A = G.dot(G.T) / max(n, 1) + np.eye(n)
  elif kind == 'illcond':
    Q, _ = np.linalg.qr(r.standard_normal((n, n)))
    d = np.logspace(0, -4 if dt == np.float32 else -10, n)
    A = (Q * d).dot(Q.T)
  elif kind == 'minij':
    i = np.arange(n)
    A = (np.minimum(i[:, None], i[None, :]) + 1).astype(np.float64)
  elif kind == 'diag':
    A = np.diag(((np.arange(n) % 7) + 1.0) ** 2)
  else:
    raise ValueError(kind)
  A = A.astype(dt)
  return np.ascontiguousarray((A + A.T) / dt.type(2))


def exact_factor(kind, n, dtype):
  """The factor of 'minij' / 'diag', exact in every float dtype."""
  if kind == 'minij':
    return np.tril(np.ones((n, n), np.dtype(dtype)))
  assert kind == 'diag'
  return np.diag(((np.arange(n) % 7) + 1.0)).astype(np.dtype(dtype))


def _ratio(res, bound):
  """max res / bound; an entry whose bound is 0 must have residual 0."""
  zero = bound == 0
  assert not np.any(res[zero] != 0), 'a nonzero residual where the bound is exactly 0'
  if np.all(zero):
    return 0.0
  return float(np.max(res[~zero] / bound[~zero]))


def potrf_ratio(A, L):
  """max over the lower triangle of |A - L L^T| / (gamma_{n+1} |L| |L|^T)."""
  dt = A.dtype
  _wide(dt)
  n = A.shape[0]
  assert np.all(np.isfinite(L)), 'the factor has non-finite entries'
  assert not np.any(np.triu(L, 1)), 'the factor is not zero above the diagonal'
  l = L.astype(LD)
  al = np.abs(l)
  a = A.astype(LD)
  worst, bs = 0.0, 256
  for i0 in range(0, n, bs):  # block (i, j <= i) of the lower triangle: columns past the block's end are zero
    for j0 in range(0, i0 + 1, bs):
      i1, j1 = min(n, i0 + bs), min(n, j0 + bs)
      res = np.abs(a[i0:i1, j0:j1] - l[i0:i1, :j1].dot(l[j0:j1, :j1].T))
      bound = gamma(n + 1, dt) * al[i0:i1, :j1].dot(al[j0:j1, :j1].T)
      keep = np.arange(i0, i1)[:, None] >= np.arange(j0, j1)[None, :]
      worst = max(worst, _ratio(res[keep], bound[keep]))
  return worst


def solve_ratio(L, X, Bm, side, trans):
  """max |op(L) X - B| / (gamma_n |L| |X|) (side 'L'; side 'R': X op(L) = B)."""
  dt = L.dtype
  _wide(dt)
  assert np.all(np.isfinite(X)), 'the solution has non-finite entries'
  l = np.tril(L).astype(LD)
  op = l.T if trans else l
  x, b = X.astype(LD), Bm.astype(LD)
  g = gamma(max(L.shape[0], 1), dt)
  if side == 'L':
    return _ratio(np.abs(op.dot(x) - b), g * np.abs(op).dot(np.abs(x)))
  return _ratio(np.abs(x.dot(op) - b), g * np.abs(x).dot(np.abs(op)))


def syrk_ratio(C0, A, Bm, C, lower=False):
  """max |C0 - A B^T - C| / (gamma_{K+1} (|C0| + |A| |B|^T)); ``lower``: over
  the lower triangle only (whatever C0 and C hold above it)."""
  dt = A.dtype
  _wide(dt)
  a, b = A.astype(LD), Bm.astype(LD)
  keep = np.tril(np.ones(C.shape, bool)) if lower else np.ones(C.shape, bool)
  c0 = C0.astype(LD)[keep]
  assert np.all(np.isfinite(C[keep])), 'the result has non-finite entries'
  res = np.abs(c0 - a.dot(b.T)[keep] - C.astype(LD)[keep])
  bound = gamma(A.shape[1] + 1, dt) * (np.abs(c0) + np.abs(a).dot(np.abs(b).T)[keep])
  return _ratio(res, bound)


def assert_bound(ratio, what):
  print('%s: ratio to the bound %.4g' % (what, ratio))
  assert ratio <= 1.0, '%s: %.4g times the derived bound' % (what, ratio)


class LinalgFakeBackend(TopkFakeBackend):
  """TopkFakeBackend + scipy ``potrf`` / ``trsm`` / ``syrk``."""

  def potrf(self, A, L):
    from scipy.linalg import lapack
    a = _np(A)
    assert a.ndim == 2 and a.shape[0] == a.shape[1] and tuple(L.shape) == a.shape and L.dtype == A.dtype
    assert a.dtype in (np.float32, np.float64)
    f = lapack.spotrf if a.dtype == np.float32 else lapack.dpotrf
    info = 0
    c = np.zeros_like(a)
    if a.shape[0]:
      with np.errstate(all='ignore'):
        c, info = f(np.tril(a), lower=1, clean=1, overwrite_a=0)
      nan = np.nonzero(np.isnan(np.diag(c)))[0]
      if info == 0 and nan.size:  # the contract counts a NaN pivot as a failure; not every LAPACK build does
        info = int(nan[0]) + 1
    _put(L, np.tril(c))
    self.calls.append('potrf')
    return torch.tensor([info], dtype=torch.int32)

  def trsm(self, L, Bm, side='L', trans=False):
    from scipy.linalg import solve_triangular
    assert side in ('L', 'R')
    l, b = _np(L), _np(Bm)
    assert l.ndim == 2 and b.ndim == 2 and l.dtype == b.dtype and l.dtype in (np.float32, np.float64)
    nl = b.shape[0] if side == 'L' else b.shape[1]
    assert l.shape == (nl, nl)
    if b.size:
      with np.errstate(all='ignore'):
        if side == 'L':
          x = solve_triangular(l, b, trans=1 if trans else 0, lower=True, check_finite=False)
        else:  # X op(L) = B  <=>  op(L)^T X^T = B^T
          x = solve_triangular(l, b.T, trans=0 if trans else 1, lower=True, check_finite=False).T
      _put(Bm, x.astype(b.dtype))
    self.calls.append('trsm')

  def syrk(self, A, Bm, C, lower=False):
    a, b, c = _np(A), _np(Bm), _np(C)
    assert a.ndim == b.ndim == c.ndim == 2 and a.shape[1] == b.shape[1] and c.shape == (a.shape[0], b.shape[0])
    assert a.dtype == b.dtype == c.dtype and a.dtype in (np.float32, np.float64)
    r = c - a.dot(b.T)
    if lower:
      assert c.shape[0] == c.shape[1]
      r = np.where(np.tril(np.ones(c.shape, bool)), r, c)
    _put(C, r.astype(c.dtype))
    self.calls.append('syrk')

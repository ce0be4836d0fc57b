"""The yardsticks and the inputs of the pairwise-kernel tests,
and the CPU test double's ``pairwise``.

``pairwise_ref`` evaluates, in NumPy float64 and LITERALLY as the formulas read
(differences, squares or absolute values, sums over the features),

    sqeuclidean s_ij = sum_k (x_ik - y_jk)^2,   euclidean sqrt(s_ij),
    manhattan sum_k |x_ik - y_jk|,              rbf exp(-gamma s_ij),

chunked over the rows so that no (chunk, m, d) block is larger than a few MB.
Beside the value it returns ``gamma s_ij`` (zeros for the other metrics): exp
amplifies the relative error of s by that much, so it enters the bound.

THE BOUND.  Each of the d terms of a sum costs at most three roundings (the
difference, the square, the addition; the kernel fuses the last two), the sum
about d more in the worst case; sqrt halves a relative error, exp multiplies
it by gamma s.  With u the unit roundoff, while (d + 4) u < TOL,

    |got - ref| <= TOL (1 + gamma s_ij) |ref| + tiny

bounds every metric: TOL is the project's 1e-5 (float32) / 1e-12 (float64), so
d <= 130 keeps (d + 4) u at 8e-6 / 1.5e-14, and ``tiny`` is the dtype's
smallest normal (a result below it may be flushed to 0).  For the degrees
D_i = sum_j a_ij the bound is the sum of the elements' bounds over the row (all
terms are >= 0, so the summation itself adds at most (m - 1) u relative to the
sum even in plain float32, and the kernel carries it in float64); for
L_ij = a_ij / sqrt(D_i D_j) the factor is doubled for the two scales.
"""
import numpy as np
import torch

from eigh_ref import EighFakeBackend, canonical, lapack_eigh
from fake_backend import _np

TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
METRICS = ('sqeuclidean', 'euclidean', 'manhattan', 'rbf')
CHUNK_BYTES = 4 << 20
D_MAX = 130  # (d + 4) u < TOL holds up to here with room


def pair_sums(X, Y):
  """(s, l1): float64 (n, m) sums of the squared and of the absolute
  differences of the rows of X and Y as stored (widened to float64)."""
  X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
  n, m, d = X.shape[0], Y.shape[0], X.shape[1]
  assert Y.shape[1] == d
  s, l1 = np.zeros((n, m)), np.zeros((n, m))
  chunk = max(1, CHUNK_BYTES // (8 * max(m * d, 1)))
  with np.errstate(invalid='ignore', over='ignore'):
    for lo in range(0, n, chunk):
      diff = X[lo:lo + chunk, None, :] - Y[None, :, :]
      s[lo:lo + chunk] = np.square(diff).sum(axis=2)
      l1[lo:lo + chunk] = np.abs(diff).sum(axis=2)
  return s, l1


def from_sums(s, l1, metric, gamma):
  """(value, gamma s) of ``metric`` from ``pair_sums``' answer."""
  with np.errstate(invalid='ignore', over='ignore', under='ignore'):
    if metric == 'sqeuclidean':
      return s, np.zeros_like(s)
    if metric == 'euclidean':
      return np.sqrt(s), np.zeros_like(s)
    if metric == 'manhattan':
      return l1, np.zeros_like(s)
    assert metric == 'rbf', metric
    gs = gamma * s
    return np.exp(-gs), gs


def pairwise_ref(X, Y, metric, gamma=1.0):
  """(value, gamma s): the float64 (n, m) yardstick of ``metric``."""
  return from_sums(*pair_sums(X, X if Y is None else Y), metric, gamma)


def bound(ref, gs, dtype, factor=1.0):
  """The elementwise error bound of the module docstring."""
  dt = np.dtype(dtype)
  with np.errstate(invalid='ignore'):
    return factor * TOL[dt] * (1.0 + gs) * np.abs(ref) + np.finfo(dt).tiny


def inv_sqrt_degrees(D):
  with np.errstate(divide='ignore', invalid='ignore'):
    return np.where(D == 0, 1.0, 1.0 / np.sqrt(D))


def affinity_ref(X, metric, gamma=1.0, diagonal=1.0):
  """(L, D, A, gamma s): the float64 yardstick of ``normalized_affinity`` and
  the unscaled matrix it comes from."""
  A, gs = pairwise_ref(X, None, metric, gamma)
  D = A.sum(axis=1)
  sc = inv_sqrt_degrees(D)
  L = A * (sc[:, None] * sc[None, :])
  L[np.arange(L.shape[0]), np.arange(L.shape[0])] = diagonal
  return L, D, A, gs


def assert_within(got, ref, gs, dtype, what, factor=1.0):
  """got (any float dtype) against the float64 yardstick, NaN where it has NaN."""
  got = np.asarray(got, np.float64)
  assert got.shape == ref.shape, (what, got.shape, ref.shape)
  nan = np.isnan(ref)
  assert np.array_equal(np.isnan(got), nan), (what, 'NaN pattern')
  err = np.where(nan, 0.0, np.abs(got - np.where(nan, 0.0, ref)))
  lim = np.where(nan, 1.0, bound(ref, gs, dtype, factor))
  worst = float((err / lim).max()) if err.size else 0.0
  assert worst <= 1.0, '%s: error / bound = %.3g' % (what, worst)
  return worst


def assert_degrees_within(got, A, gs, dtype, what):
  """Row sums against sum_j a_ij: the elements' bounds summed over the row."""
  got = np.asarray(got, np.float64)
  ref, lim = A.sum(axis=1), bound(A, gs, dtype).sum(axis=1)
  assert got.shape == ref.shape, (what, got.shape)
  worst = float((np.abs(got - ref) / lim).max()) if ref.size else 0.0
  assert worst <= 1.0, '%s: degree error / bound = %.3g' % (what, worst)
  return worst


def float32_model(X, Y, metric, gamma):
  """The difference form evaluated in plain float32 NumPy, k ascending, three
  roundings a term: what the bound must hold for before any kernel is judged
  by it."""
  X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
  acc = np.zeros((X.shape[0], Y.shape[0]), np.float32)
  for k in range(X.shape[1]):
    diff = X[:, k, None] - Y[None, :, k]
    acc = acc + (np.abs(diff) if metric == 'manhattan' else diff * diff)
  if metric == 'euclidean':
    acc = np.sqrt(acc)
  if metric == 'rbf':
    acc = np.exp(np.float32(-gamma) * acc)
  assert acc.dtype == np.float32
  return acc


# ------------------------------------------------------------------ inputs
def gamma_for(d):
  """gamma s is about 1 for standard-normal points (s is about 2 d)."""
  return 0.5 / d


def points(n, d, dtype, seed):
  return np.random.RandomState(seed).standard_normal((n, d)).astype(dtype)


def blobs(n, d, k, dtype=np.float64, seed=7, spread=0.15, distance=4.0):
  """(points (n, d), labels (n,)): k well-separated Gaussian blobs of n / k
  points each, centres ``distance`` apart along a line bent through the first
  two features, shuffled."""
  r = np.random.RandomState(seed)
  labels = np.arange(n) % k
  centres = np.zeros((k, d))
  centres[:, 0] = distance * np.arange(k)
  if d > 1:
    centres[:, 1] = distance * (np.arange(k) % 2)
  pts = centres[labels] + spread * r.standard_normal((n, d))
  order = r.permutation(n)
  return pts[order].astype(dtype), labels[order]


def same_partition(a, b):
  """Are the label vectors a and b equal up to a relabelling?"""
  a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
  pairs = set(zip(a.tolist(), b.tolist()))
  return a.shape == b.shape and len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def edge_shapes(tb, kc):
  """The (n, m, d) of the kernel's edge-shape tests for tile edge ``tb`` and
  k-chunk ``kc``: n and m around one tile and at 2 tb + 3, n != m among them,
  d at 1, around the chunk and at D_MAX."""
  edges = (tb - 1, tb, tb + 1, 2 * tb + 3)
  ds = (1, kc - 1, kc, kc + 1, D_MAX)
  shapes = [(n, m, kc + 1) for n in edges for m in edges]  # every edge pair at a d with a partial second chunk
  shapes += [(tb + 1, 2 * tb + 3, d) for d in ds] + [(2 * tb + 3, tb - 1, d) for d in ds]
  return shapes


# ------------------------------------------------------ the driver's model
def lanczos_model(A, rank):
  """examples.lanczos.solve for a symmetric A, typed out in NumPy, with the
  project's sign rule for the eigenvectors of the tridiagonal matrix."""
  rank += 2
  n = A.shape[1]
  v_next, v_prev = np.ones(n) / np.sqrt(n), np.zeros(n)
  beta, alpha, V = np.zeros(rank + 1), np.zeros(rank), np.zeros((n, rank))
  for i in range(rank):
    w = A.dot(v_next)
    alpha[i] = np.dot(w, v_next)
    w = w - alpha[i] * v_next - beta[i] * v_prev
    for t in range(i):
      w -= np.dot(w, V[:, t]) * V[:, t]
    beta[i + 1] = np.linalg.norm(w, 2)
    v_prev, v_next = v_next, w / beta[i + 1]
    V[:, i] = v_prev
  T = np.diag(alpha) + np.diag(beta[1:rank], 1) + np.diag(beta[1:rank], -1)
  d, v = canonical(*lapack_eigh(T))
  idx = np.argsort(np.absolute(d))[::-1]
  return d[idx][:rank - 2], np.dot(V, v[:, idx])[:, :rank - 2]


def spectral_model(pts, k, num_iter, metric):
  """The driver's chain in NumPy float64: (labels, U, initial centres)."""
  L = affinity_ref(pts, metric, 1.0, 1.0)[0]
  _d, U = lanczos_model(L, min(2 * k, pts.shape[0]))
  U = U[:, :k]
  centres = U[np.argmax(U, axis=0)]
  init = centres.copy()
  rng = np.random.default_rng(0)  # KMeans' seed: an empty cluster is re-seeded from it, as in examples.kmeans
  for _ in range(num_iter):
    dist = np.square(U[:, None, :] - centres[None, :, :]).sum(axis=2)
    labels = dist.argmin(axis=1)
    counts = np.bincount(labels, minlength=k)
    centres = np.stack([U[labels == c].sum(axis=0) for c in range(k)])
    empty = counts == 0
    if np.any(empty):
      counts[empty] = 1
      centres[empty, :] = rng.standard_normal((np.count_nonzero(empty), k))
    centres = centres / counts.reshape(k, 1)
  return labels, U, init


# -------------------------------------------------------------- test double
class AffinityFakeBackend(EighFakeBackend):
  """The CPU test double + ``pairwise`` by the yardstick; ``pairwise_calls``
  records (n, m, out wanted, row_sums wanted, diag_col0) of every call."""

  def __init__(self):
    EighFakeBackend.__init__(self)
    self.pairwise_calls = []

  def pairwise(self, X, Y, metric, gamma, out=None, row_sums=None, row_scale=None, col_scale=None, diag_col0=-1,
               diag_value=0.0, splits=None):
    x, y = _np(X), _np(Y)
    dt = x.dtype
    assert dt in (np.float32, np.float64) and y.dtype == dt and x.ndim == y.ndim == 2 and x.shape[1] == y.shape[1]
    assert metric in METRICS and (row_scale is None) == (col_scale is None)
    want_out, want_sums = out is not None and out is not False, row_sums is not None and row_sums is not False
    assert want_out or want_sums
    a = pairwise_ref(x, y, metric, gamma)[0]
    if row_scale is not None:
      r, c = _np(row_scale), _np(col_scale)
      assert r.shape == (x.shape[0],) and c.shape == (y.shape[0],) and r.dtype == c.dtype == dt
      a = a * (r[:, None].astype(np.float64) * c[None, :].astype(np.float64))
    sums = a.sum(axis=1)
    if diag_col0 >= 0:
      i = np.arange(x.shape[0])
      keep = diag_col0 + i < y.shape[0]
      a[i[keep], diag_col0 + i[keep]] = diag_value
    self.calls.append('pairwise')
    self.pairwise_calls.append((x.shape[0], y.shape[0], want_out, want_sums, int(diag_col0)))
    return (torch.as_tensor(a.astype(dt)) if want_out else None,
            torch.as_tensor(sums.astype(dt)) if want_sums else None)

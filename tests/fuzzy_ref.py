"""The yardstick and the inputs of the fuzzy k-means tests, and
the CPU test double's ``fuzzy_step``.

``membership_k2`` evaluates the membership in the K^2 form LITERALLY, in
float64: ``u_ij = 1 / sum_l (d_ij / d_il)^e`` with ``d = |x - c|^2 + eps``.
``membership_ok`` is the O(K) form the kernel uses, ``(dmin / d)^e`` normalised;
the host tests hold the two together.  ``fuzzy_ref`` adds the labels, counts
and sums; ``fuzzy_kmeans_loop`` is the NumPy model of the driver.
"""
import numpy as np
import torch

from fake_backend import FakeBackend

# (N, D, K, m) of the GPU tests
SHAPES = [(1, 1, 1, 2.0), (67, 5, 3, 2.0), (300, 33, 17, 2.0), (129, 128, 256, 1.5), (200, 7, 64, 3.0),
          (257, 130, 65, 1.1)]


def _np(t):
  return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def sq_dist(X, C, eps):
  """float64 (n, k): sum_c (x_c - c_c)^2 + eps, in the difference form."""
  X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
  return ((X[:, None, :] - C[None, :, :]) ** 2).sum(axis=2) + eps


def membership_k2(d, e):
  """(n, k): 1 / sum_l (d_j / d_l)^e, typed out as the (n, k, k) ratio; huge
  ratios may overflow to +inf, whose reciprocal is the right answer 0."""
  with np.errstate(over='ignore'):
    return 1.0 / ((d[:, :, None] / d[:, None, :]) ** e).sum(axis=2)


def membership_ok(d, e):
  """(n, k): the same in O(K) per row and without overflow."""
  t = (d.min(axis=1, keepdims=True) / d) ** e
  return t / t.sum(axis=1, keepdims=True)


def fuzzy_ref(X, C, exponent, eps=1e-11, weight_power=1.0):
  """dict of float64 ``dist`` (n, k), ``U`` (n, k), ``labels`` (n,) int64,
  ``counts`` (k,), ``sums`` (k, d) of the inputs as stored (any float dtype)."""
  X64 = np.asarray(X, np.float64)
  d = sq_dist(X64, C, eps)
  U = membership_k2(d, exponent)
  W = U ** weight_power
  return {'dist': d, 'U': U, 'labels': np.argmin(d, axis=1).astype(np.int64), 'counts': W.sum(axis=0),
          'sums': W.T @ X64}


def fuzzy_data(N, D, K, dtype, seed=7, plant=True):
  """(X (N, D) in ``dtype``, C (K, D) float64) from one seed; with ``plant``
  row 3 of X is centre 0 (as far as dtype holds it): its distance is eps."""
  r = np.random.RandomState(seed)
  X = r.randn(N, D).astype(dtype)
  C = r.randn(K, D)
  if plant and N > 3:
    C[0] = X[3].astype(np.float64)
  return X, C


def fuzzy_blobs(N, D, K, dtype, seed=7):
  """(X, C) with row i of X a draw around centre i mod K, the centres far apart
  against the spread: over hundreds of thousands of rows plain Gaussian points
  always hold a near tie of the two nearest centres, these never do."""
  r = np.random.RandomState(seed)
  C = 3.0 * r.randn(K, D)
  X = (C[np.arange(N) % K] + 0.3 * r.randn(N, D)).astype(dtype)
  return X, C


def top_two_gap(d):
  """The smallest relative gap between a row's two smallest distances (+inf for k = 1)."""
  if d.shape[1] < 2:
    return np.inf
  s = np.sort(d, axis=1)
  return float(((s[:, 1] - s[:, 0]) / s[:, 1]).min())


def fuzzy_kmeans_loop(X, C, m, num_iter, weight_power=1.0):
  """(labels, centres) of ``num_iter`` iterations without an empty cluster."""
  X64, C = np.asarray(X, np.float64), np.array(C, np.float64)
  labels = None
  for _ in range(num_iter):
    d = ((X64[:, None, :] - C[None, :, :]) ** 2).sum(axis=2) + 1e-11
    U = 1.0 / ((d[:, :, None] / d[:, None, :]) ** (2.0 / (m - 1.0))).sum(axis=2)
    W = U ** weight_power
    labels = np.argmin(d, axis=1)
    counts = W.sum(axis=0)
    assert np.all(counts > 0)
    C = (W.T @ X64) / counts[:, None]
  return labels, C


# -------------------------------------------------------------- test double
class FuzzyFakeBackend(FakeBackend):
  """The CPU test double + ``fuzzy_step`` by the yardstick.  ``zero_counts``:
  centre indices whose counts and sums are reported as zero (the driver's
  reseeding branch)."""
  zero_counts = ()

  def fuzzy_step(self, points, centers, exponent, eps, weight_power, want_labels, want_U, sums=None, counts=None):
    p, c = _np(points), _np(centers)
    assert p.ndim == 2 and p.dtype in (np.float32, np.float64) and c.dtype == np.float64 and c.shape[1] == p.shape[1]
    assert (sums is None) == (counts is None)
    r = fuzzy_ref(p, c, exponent, eps, weight_power)
    s, n = r['sums'].copy(), r['counts'].copy()
    for j in self.zero_counts:
      s[j], n[j] = 0.0, 0.0
    if sums is not None:
      s, n = s + _np(sums), n + _np(counts)
    self.calls.append('fuzzy_step')
    return (torch.as_tensor(r['labels']) if want_labels else None,
            torch.as_tensor(r['U'].astype(p.dtype)) if want_U else None, torch.as_tensor(s), torch.as_tensor(n))

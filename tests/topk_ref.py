"""Shared by tests/test_topk.py and tests/test_topk_gpu.py: the NumPy oracle of
the topk / knn contract, the CPU test double's ``topk`` /
``knn`` (HipBackend's signatures) and the nearest-neighbour data generators.
The topk data are sort_ref.sort_data's."""
import numpy as np

from spartan_amd import backend as B
from fake_backend import _np, _put
from sort_ref import SortFakeBackend, sort_data  # noqa: F401  (sort_data: re-exported)


def order_ref(x, axis, largest):
  """The full stable order along ``axis``: positions, ascending
  (np.argsort(kind='stable')), or for ``largest`` descending with equal keys
  lower position first and NaNs last (-x for floats, ~x for ints / bool)."""
  x = np.asarray(x)
  if largest:
    x = -x if x.dtype.kind == 'f' else ~x
  return np.argsort(x, axis=axis, kind='stable').astype(np.int64)


def topk_ref(x, k, axis=-1, largest=False):
  """(values, positions) of the first k along ``axis``."""
  x = np.asarray(x)
  idx = np.take(order_ref(x, axis, largest), np.arange(k), axis=axis)
  return np.take_along_axis(x, idx, axis), idx


def knn_sums(X, q):
  """s[i, j]: the fp64 sum over d, in order, of (double(q[i, d]) - double(X[j, d]))^2,
  every operation rounded separately, the accumulator starting at +0.0."""
  X = np.asarray(X, dtype=np.float64)
  q = np.asarray(q, dtype=np.float64)
  s = np.zeros((q.shape[0], X.shape[0]), np.float64)
  with np.errstate(all='ignore'):
    for d in range(X.shape[1]):
      df = q[:, d][:, None] - X[:, d][None, :]
      sq = df * df
      s = s + sq
  return s


def knn_ref(X, q, k):
  """(s, ind): per query the first k of the order (s, index) ascending, NaN
  sums after +inf."""
  s = knn_sums(X, q)
  ind = np.argsort(s, axis=1, kind='stable')[:, :k].astype(np.int64)
  return np.take_along_axis(s, ind, 1), ind


def same_bits(got, want):
  """Bit-for-bit equality of two float arrays, NaNs matching NaNs (their
  payloads are not part of the contract)."""
  got, want = np.asarray(got), np.asarray(want)
  if got.shape != want.shape or got.dtype != want.dtype:
    return False
  if got.dtype.kind != 'f':
    return bool(np.array_equal(got, want))
  ut = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
  gn, wn = np.isnan(got), np.isnan(want)
  return bool(np.array_equal(gn, wn) and np.array_equal(got.view(ut)[~gn], want.view(ut)[~wn]))


class TopkFakeBackend(SortFakeBackend):
  """SortFakeBackend + NumPy ``topk`` / ``knn``."""

  def topk(self, src, in_idx, out_vals, out_idx, axis_geom, k, largest=False):
    o, n, i = (int(v) for v in axis_geom)
    k = int(k)
    assert src.is_contiguous() and src.numel() == o * n * i
    assert out_vals is not None or out_idx is not None
    assert 1 <= k <= n and k <= B.TOPK_K_MAX
    x = _np(src).reshape(o, n, i)
    vals, idx = topk_ref(x, k, 1, largest)
    if out_vals is not None:
      assert out_vals.dtype == src.dtype and out_vals.numel() == o * k * i and out_vals.is_contiguous()
      _put(out_vals, vals)
    if out_idx is not None:
      assert B.np_dtype(out_idx.dtype) == np.int64 and out_idx.numel() == o * k * i and out_idx.is_contiguous()
      if in_idx is not None:
        assert B.np_dtype(in_idx.dtype) == np.int64 and in_idx.numel() == src.numel() and in_idx.is_contiguous()
        idx = np.take_along_axis(_np(in_idx).reshape(o, n, i), idx, 1)
      _put(out_idx, idx)
    self.calls.append('topk')

  def knn(self, points, queries, k, index_base, out_s, out_idx):
    X, q = _np(points), _np(queries)
    assert q.dtype == np.float64 and X.ndim == 2 and q.ndim == 2 and X.shape[1] == q.shape[1]
    assert 1 <= k <= X.shape[0] and k <= B.KNN_K_MAX
    assert tuple(out_s.shape) == tuple(out_idx.shape) == (q.shape[0], k)
    s, ind = knn_ref(X, q, k)
    _put(out_s, s)
    _put(out_idx, ind + int(index_base))
    self.calls.append('knn')


def knn_data(kind, N, Q, D, dtype, seed):
  """(X, q) of ``dtype``.  kind:
    'grid'       integer coordinates in [0, 3]: every sum exact, ties everywhere;
    'uniform'    U(0, 1);
    'dup'        every point present three times (N rounded down to what fits,
                 the rest uniform);
    'far'        1e6 + U(0, 1) in float32, 1e9 + U(0, 1) in float64: the
                 |q|^2 + |x|^2 - 2 q.x expansion loses every digit here;
    'nonfinite'  uniform with about 5 % of the points carrying a NaN or an inf
                 coordinate."""
  r = np.random.RandomState(seed)
  dt = np.dtype(dtype)
  if kind == 'grid':
    return r.randint(0, 4, (N, D)).astype(dt), r.randint(0, 4, (Q, D)).astype(dt)
  X = r.random_sample((N, D))
  q = r.random_sample((Q, D))
  if kind == 'dup' and N >= 3:
    m = N // 3
    X[m:2 * m] = X[:m]
    X[2 * m:3 * m] = X[:m]
  elif kind == 'far':
    off = 1e6 if dt == np.float32 else 1e9
    X, q = X + off, q + off
  elif kind == 'nonfinite':
    bad = np.nonzero(r.random_sample(N) < 0.05)[0]
    X[bad, r.randint(0, D, bad.size)] = r.choice([np.nan, np.inf, -np.inf], bad.size)
  else:
    assert kind in ('uniform', 'dup'), kind
  return X.astype(dt), q.astype(dt)

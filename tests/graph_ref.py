"""The yardstick and the inputs of the shortest-path tests, and
the CPU test double's ``apsp``.

``apsp_ref`` is scipy's Dijkstra on the float64 image of the dtype-rounded
weights, after the edge rules of spx_apsp applied in NumPy; ``fw_numpy`` is a
plain Floyd-Warshall that cross-checks it.  ``isomap_model`` is the NumPy model
of ``examples.isomap.Isomap``.
"""
import numpy as np
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import shortest_path as _scipy_shortest_path

from eigh_ref import EighFakeBackend
from sparse_ref import SparseFakeBackend

KINDS = ('int', 'knn', 'chain', 'empty')


def _np(t):
  return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ------------------------------------------------------------- the yardstick
def edge_weights(G, directed):
  """float64 (n, n): the weight of the edge i -> j, +inf where there is none,
  0 on the diagonal -- the rules of spx_apsp on the matrix ``G`` as stored."""
  W = np.asarray(G).astype(np.float64)
  n = W.shape[0]
  with np.errstate(invalid='ignore'):
    W = np.where(np.isfinite(W) & (W > 0), W, np.inf)
  if not directed:
    W = np.minimum(W, W.T)
  W[np.arange(n), np.arange(n)] = 0.0
  return W


def has_bad_weight(G):
  """spx_apsp's info == -1: a negative, -inf or NaN entry anywhere."""
  g = np.asarray(G)
  with np.errstate(invalid='ignore'):
    return bool(np.any(~(g >= 0)))


def apsp_ref(G, directed=True, unreachable=np.inf):
  """float64 (n, n) shortest path lengths of ``G`` (any float dtype; its values
  are taken as stored), ``unreachable`` where there is no path."""
  W = edge_weights(G, directed)
  n = W.shape[0]
  if n == 0:
    return W
  A = np.where(np.isfinite(W), W, 0.0)  # dense zeros are scipy's "no edge"
  D = _scipy_shortest_path(sp.csr_matrix(A), method='D', directed=True)
  D = np.asarray(D, np.float64)
  D[np.arange(n), np.arange(n)] = 0.0
  return np.where(np.isinf(D), float(unreachable), D)


def fw_numpy(G, directed=True):
  """Plain Floyd-Warshall in float64 on the same edge rules: n passes."""
  D = edge_weights(G, directed)
  for k in range(D.shape[0]):
    D = np.minimum(D, D[:, k:k + 1] + D[k:k + 1, :])
  return D


# ----------------------------------------------------------------- the inputs
def swiss_roll(n, seed=0, dtype=np.float64):
  """(n, 3): a seeded swiss roll."""
  r = np.random.RandomState(seed)
  t = 1.5 * np.pi * (1 + 2 * r.rand(n))
  y = 21 * r.rand(n)
  return np.stack([t * np.cos(t), y, t * np.sin(t)], axis=1).astype(dtype)


def knn_lists(X, k):
  """(dist, ind) of the k nearest rows of X to each row of X, nearest first,
  ties by index (NearestNeighbors' order): selection on the float64 sum of
  squares, dist rounded once to X's dtype."""
  X64 = np.asarray(X, np.float64)
  s = ((X64[:, None, :] - X64[None, :, :]) ** 2).sum(axis=2)
  ind = np.argsort(s, axis=1, kind='stable')[:, :k]
  dist = np.sqrt(np.take_along_axis(s, ind, axis=1)).astype(X.dtype)
  return dist, ind


def knn_graph(X, n_neighbors):
  """Dense (n, n) float64 matrix of the directed n_neighbors graph of X as
  Isomap builds it: n_neighbors + 1 lists, the own index dropped where present,
  else the last column."""
  n = X.shape[0]
  n_neighbors = min(n_neighbors, n - 1)  # a tiny input: everyone else
  dist, ind = knn_lists(X, n_neighbors + 1)
  G = np.zeros((n, n), np.float64)
  for i in range(n):
    cols = list(ind[i])
    drop = cols.index(i) if i in cols else n_neighbors
    for c in range(n_neighbors + 1):
      if c != drop:
        G[i, ind[i, c]] = dist[i, c]
  return G


def graph_data(kind, n, dtype, seed=0, weight=1.0):
  """The (n, n) edge-weight matrix of ``kind`` in ``dtype``."""
  dtype = np.dtype(dtype)
  if kind == 'empty':
    return np.zeros((n, n), dtype)
  if kind == 'chain':
    G = np.zeros((n, n), dtype)
    i = np.arange(n - 1)
    G[i, i + 1] = weight
    return G
  if kind == 'int':
    r = np.random.RandomState(seed)
    mask = r.rand(n, n) < min(1.0, 3.5 / max(n, 1))
    G = np.where(mask, r.randint(1, 50, size=(n, n)), 0).astype(dtype)
    G[np.arange(n), np.arange(n)] = 0
    return G
  if kind == 'knn':
    return knn_graph(swiss_roll(n, seed), 8).astype(dtype)
  raise ValueError(kind)


# -------------------------------------------------------------- Isomap model
def sign_rule(E):
  E = np.array(E, copy=True)
  for j in range(E.shape[1]):
    i = int(np.argmax(np.abs(E[:, j])))
    if E[i, j] < 0:
      E[:, j] = -E[:, j]
  return E


def isomap_model(X, n_neighbors, n_components):
  """dict of the NumPy model's ``dist``, the whole ascending spectrum ``w`` of
  the centered kernel, the top ``lam`` (descending) and ``embedding``."""
  n = X.shape[0]
  D = apsp_ref(knn_graph(X, n_neighbors), directed=False)
  K = -0.5 * D * D
  Kc = K - K.mean(axis=1, keepdims=True) - K.mean(axis=0, keepdims=True) + K.mean()
  w, V = np.linalg.eigh((Kc + Kc.T) / 2)
  lam = w[::-1][:n_components].copy()
  E = sign_rule(V[:, ::-1][:, :n_components] * np.sqrt(lam))
  return {'dist': D, 'w': w, 'lam': lam, 'embedding': E, 'n': n}


def check_isomap(model, iso, tol, what):
  """The bounds of the issue: dist within 1e-12 relative, |lam^ - lam| <= 2 tol
  lam_1, column i of the embedding within 2 tol lam_1 / gap_i sqrt(lam_i)."""
  D, w, lam, E = model['dist'], model['w'], model['lam'], model['embedding']
  nc = len(lam)
  assert np.all(np.isfinite(D))
  np.testing.assert_allclose(iso.dist_matrix_, D, rtol=1e-12, atol=0)
  assert iso.embedding_.shape == E.shape and iso.embedding_.dtype == np.float64
  lam1 = lam[0]
  desc = w[::-1]
  for i in range(nc):
    gap = min(abs(desc[i] - desc[j]) for j in range(len(desc)) if j != i)
    assert gap / lam1 > 1e-3, '%s: the gap of pair %d is %.3g lam_1: the bound would be vacuous' % (what, i, gap / lam1)
    dl = abs(iso.lambdas_[i] - lam[i])
    de = float(np.linalg.norm(sign_rule(iso.embedding_)[:, i] - E[:, i]))
    lim_l, lim_e = 2 * tol * lam1, 2 * tol * lam1 / gap * np.sqrt(lam[i])
    print('%s pair %d: |dlam| %.3g (bound %.3g), |dE| %.3g (bound %.3g), gap / lam_1 %.3g'
          % (what, i, dl, lim_l, de, lim_e, gap / lam1))
    assert dl <= lim_l, what
    assert de <= lim_e, what


# -------------------------------------------------------------- test double
class GraphFakeBackend(SparseFakeBackend, EighFakeBackend):
  """The CPU test double (FakeBackend with the neighbour, QR, eigh and sparse
  doubles the Isomap driver runs on) + ``apsp`` by ``apsp_ref``."""

  def apsp(self, G, directed=True, unreachable=float('inf')):
    g = _np(G)
    assert g.ndim == 2 and g.shape[0] == g.shape[1] and g.dtype in (np.float32, np.float64)
    info = np.array([-1 if has_bad_weight(g) else 0], np.int32)
    with np.errstate(invalid='ignore'):
      clean = np.where(g >= 0, g, 0)
    D = apsp_ref(clean, directed, unreachable).astype(g.dtype)
    self.calls.append('apsp')
    return torch.as_tensor(D), torch.as_tensor(info)

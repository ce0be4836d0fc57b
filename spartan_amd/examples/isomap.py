"""The reference's manifold learner on the MI355X path
(spartan/examples/sklearn/manifold/isomap.py): ``Isomap(n_neighbors,
n_components, eigen_solver, tol, max_iter, neighbors_algorithm).fit(X)`` sets
``embedding_`` (n, n_components), ``dist_matrix_`` (n, n) and
``training_data_``, all NumPy.

The reference chains scikit-learn's k-neighbours graph, a Cython Dijkstra per
row tile and scikit-learn's KernelPCA.  Here:

  1. neighbours: ``NearestNeighbors(n_neighbors + 1).kneighbors(X)``; from each
     row the row's own index is dropped where present, else the last column;
  2. graph: the (n, n) CSR matrix of those distances, built on the host from
     the n k numbers ``kneighbors`` returns there, ingested as a sparse array;
     ``dist_matrix_ = shortest_path(S, directed=False)`` in float64
     (spx_apsp).  Duplicate points give zero-length edges, and a zero is "no
     edge" (the reference's convention): such an edge vanishes from the graph;
  3. connectivity: a +inf entry raises ``ValueError`` (the reference would
     silently embed zeros);
  4. kernel PCA in float64 on the device: K = -0.5 D^2, double centering
     Kc = K - rowmean - colmean + mean as one map over K with ``sum(K, 0)`` and
     ``sum(K, 1)``;
  5. the top ``n_components`` eigenpairs of Kc by subspace iteration with
     Rayleigh-Ritz: Q <- qr(Kc Q)[0] on p = n_components + 8 columns from a
     fixed seed, T = Q^T Kc Q, (w, Z) = eigh(T), Ritz vectors Q Z, until every
     wanted pair has ||Kc v - lambda v||_2 <= tol_eff |lambda_1| (tol_eff = tol,
     or 1e-10 for tol = 0) or ``max_iter`` rounds (default 200) are spent.  One
     product with Kc a round: Y = Kc Q serves T, the residual and the next Q.
     ``eigen_solver='dense'`` calls ``expr.eigh(Kc)`` instead (n within the
     eigen-solver's limit); 'auto' and 'arpack' take the iteration;
  6. ``embedding_ = V sqrt(lambda)``, every column with its entry of largest
     magnitude positive (``eigh``'s rule), so the bits do not depend on the
     route.

``lambdas_`` keeps the eigenvalues, ``n_iter_`` the rounds used and
``converged_`` whether the residual test was met; rounds that run out without
it raise a ``RuntimeWarning`` and leave the last iterate.
"""
import warnings

import numpy as np

from .. import backend, expr
from .neighbors import NearestNeighbors

SOLVERS = ('auto', 'arpack', 'dense')
EXTRA = 8          # columns iterated beyond n_components
MAX_ITER = 200     # rounds when max_iter is None
TOL_DEFAULT = 1e-10
SEED = 0


def neighbor_graph(dist, ind):
  """The (n, n) scipy CSR matrix of the k-neighbours graph from ``kneighbors``'
  (dist, ind) of n_neighbors + 1 columns: per row the own index is dropped where
  present, else the last column.  float64."""
  import scipy.sparse as sp
  n, k1 = ind.shape
  own = ind == np.arange(n)[:, None]
  drop = np.where(own.any(axis=1), own.argmax(axis=1), k1 - 1)
  keep = np.arange(k1)[None, :] != drop[:, None]
  cols = ind[keep].reshape(n, k1 - 1)
  vals = np.asarray(dist, np.float64)[keep].reshape(n, k1 - 1)
  order = np.argsort(cols, axis=1, kind='stable')
  cols = np.take_along_axis(cols, order, axis=1)
  vals = np.take_along_axis(vals, order, axis=1)
  rowptr = np.arange(n + 1, dtype=np.int64) * (k1 - 1)
  return sp.csr_matrix((vals.ravel(), cols.ravel().astype(np.int32), rowptr), shape=(n, n))


def _sign_rule(E):
  """Every column with its (first) entry of largest magnitude positive."""
  E = E.copy()
  for j in range(E.shape[1]):
    i = int(np.argmax(np.abs(E[:, j])))
    if E[i, j] < 0:
      E[:, j] = -E[:, j]
  return E


class Isomap(object):
  """Isomap embedding (the reference's signature): non-linear dimensionality
  reduction through isometric mapping."""

  def __init__(self, n_neighbors=5, n_components=2, eigen_solver='auto', tol=0, max_iter=None,
               neighbors_algorithm='auto'):
    if eigen_solver not in SOLVERS:
      raise ValueError('Isomap: eigen_solver %r is not one of %s' % (eigen_solver, SOLVERS))
    self.n_neighbors = n_neighbors
    self.n_components = n_components
    self.eigen_solver = eigen_solver
    self.tol = tol
    self.max_iter = max_iter
    self.neighbors_algorithm = neighbors_algorithm
    self.nbrs_ = NearestNeighbors(n_neighbors=n_neighbors, algorithm=neighbors_algorithm)

  # ------------------------------------------------------------ the chain
  def _distances(self, X):
    k = self.n_neighbors
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
      raise ValueError('Isomap: n_neighbors %r must be a positive integer' % (k,))
    if k + 1 > backend.KNN_K_MAX:
      raise ValueError('Isomap: n_neighbors + 1 = %d exceeds KNN_K_MAX = %d' % (k + 1, backend.KNN_K_MAX))
    self.nbrs_.fit(X)
    dist, ind = self.nbrs_.kneighbors(X, int(k) + 1)
    self.nbrs_.n_neighbors = k  # kneighbors(X, k + 1) keeps its argument as the new default; nbrs_ stays at k
    S = expr.from_numpy(neighbor_graph(dist, ind))
    D = expr.shortest_path(S, directed=False).force()
    return D

  def _centered_kernel(self, D):
    n = D.shape[0]
    D = expr.lazify(D)
    K = expr.lazify((D * D * -0.5).optimized().force())
    rows = expr.reshape(expr.sum(K, axis=1), (n, 1))
    cols = expr.sum(K, axis=0)
    total = float(expr.sum(cols).glom())
    return expr.lazify((K - rows * (1.0 / n) - cols * (1.0 / n) + total / (float(n) * n)).optimized().force())

  def _top_dense(self, Kc, nc):
    n = Kc.shape[0]
    nmax, _ = backend.syevj_plan(np.float64)
    if n > nmax:
      raise NotImplementedError("Isomap: eigen_solver='dense' holds n <= %d (the eigen-solver's limit), got n = %d; "
                                "use 'auto'" % (nmax, n))
    w, V = expr.eigh(Kc)
    w, V = w.glom(), V.glom()
    self.n_iter_ = 0
    self.converged_ = True
    return w[::-1][:nc].copy(), V[:, ::-1][:, :nc].copy()

  def _top_iterated(self, Kc, nc):
    n = Kc.shape[0]
    p = nc + EXTRA
    pmax = min(backend.geqr_plan(np.float64, p)[0], backend.syevj_plan(np.float64)[0])
    if p > n or p > pmax:
      raise ValueError('Isomap: n_components + %d = %d columns are iterated, which exceeds %s'
                       % (EXTRA, p, 'the %d points' % n if p > n else 'the limit of %d' % pmax))
    tol = float(self.tol) if self.tol and self.tol > 0 else TOL_DEFAULT
    rounds = MAX_ITER if self.max_iter is None else int(self.max_iter)
    Q = expr.lazify(expr.qr(np.random.RandomState(SEED).standard_normal((n, p)))[0].force())
    lam, V = None, None
    self.n_iter_ = 0
    self.converged_ = False
    for it in range(max(rounds, 1)):
      Y = expr.lazify(expr.dot(Kc, Q).force())
      w, Z = expr.eigh(expr.dot(expr.transpose(Q), Y))
      w = w.glom()                               # ascending; the wanted ones are the last nc
      Zt = np.ascontiguousarray(Z.glom()[:, ::-1][:, :nc])
      lam = w[::-1][:nc].copy()
      Vx = expr.dot(Q, Zt)
      R = expr.dot(Y, Zt) - Vx * lam
      res = np.sqrt(expr.sum(R * R, axis=0).glom())
      V = Vx
      self.n_iter_ = it + 1
      if np.all(res <= tol * abs(lam[0])):
        self.converged_ = True
        break
      Q = expr.lazify(expr.qr(Y)[0].force())
    if not self.converged_:
      warnings.warn('Isomap: the subspace iteration spent its %d rounds with a residual of %.3g |lambda_1| '
                    '(tol %.3g); the embedding is the last iterate' % (self.n_iter_, float(res.max() / abs(lam[0])),
                                                                      tol), RuntimeWarning, stacklevel=3)
    return lam, V.glom()

  def fit(self, X):
    """Fit the model from the (n_samples, n_features) data ``X`` (a NumPy array,
    an array or an expression).  Returns self."""
    nc = self.n_components
    if isinstance(nc, bool) or not isinstance(nc, (int, np.integer)) or nc < 1:
      raise ValueError('Isomap: n_components %r must be a positive integer' % (nc,))
    Xe = expr.from_numpy(X) if isinstance(X, np.ndarray) else expr.as_array(X)
    self.training_data_ = X if isinstance(X, np.ndarray) else Xe.glom()
    D = self._distances(Xe)
    self.dist_matrix_ = D.glom()
    far = int(np.count_nonzero(np.isinf(self.dist_matrix_)))
    if far:
      raise ValueError('Isomap: the neighbour graph is not connected: %d pairs of points are unreachable with '
                       'n_neighbors = %d; raise n_neighbors' % (far, self.n_neighbors))
    Kc = self._centered_kernel(D)
    lam, V = (self._top_dense if self.eigen_solver == 'dense' else self._top_iterated)(Kc, int(nc))
    self.lambdas_ = lam
    self.embedding_ = _sign_rule(V * np.sqrt(np.maximum(lam, 0.0)))
    return self

"""``pairwise_kernel`` and ``normalized_affinity``: the affinity matrix of a
point set and its normalised form on spx_pairwise.

The reference's spectral clustering (spartan/examples/spectral_clustering.py)
builds both by ``shuffle``: ``_row_similarity_mapper`` fills the (n, n)
affinity matrix in a Python double loop over pairs, and ``_laplacian_mapper``
scales it to D^-1/2 A D^-1/2 with a unit diagonal.  Neither needs ``shuffle``:
both are fixed computations, and one kernel serves them.

``pairwise_kernel(X, Y=None, metric, gamma)`` is the lazy (n, m) matrix of

    sqeuclidean s_ij = sum_k (x_ik - y_jk)^2,   euclidean sqrt(s_ij),
    manhattan sum_k |x_ik - y_jk|,              rbf exp(-gamma s_ij),

evaluated in the difference form: equal rows give exactly 0 (rbf: 1) and with
``Y = X`` the matrix is bitwise symmetric.

``normalized_affinity(X, metric, gamma, diagonal)`` is a lazy pair ``(L, D)``
hanging off one node: D_i = sum_j a_ij, L_ij = a_ij / sqrt(D_i D_j) with the
diagonal set to ``diagonal`` (a row of degree 0 is scaled by 1, as in the
reference).  Two launches of the one kernel per row slab: a degree pass that
stores nothing, then the scaled pass.  The (n, n) matrix A is never stored.

Routes; every rank issues the same exchanges whether or not it owns rows:

  * Y (or X as its own partner) is gathered in full to every rank
    (``blocks.whole``);
  * replicated operands are computed whole on every rank; the results are
    replicated;
  * otherwise the rows are cut at X's row cuts (``blocks.slabs``); the owner
    of a slab's first tile issues one launch for it; the results are tiled in
    row slabs on those owners;
  * for ``normalized_affinity`` the degree vector is gathered in full between
    the two passes.

Not built: ``scaled_euclidean`` (the reference's function of that name does not
compute what its docstring says: tests/test_affinity.py pins it), cosine and
other metrics, an MFMA Gram-form path, sparse points, a Y too large to
replicate on one GPU.
"""
import numpy as np

from .. import backend, runtime
from ..array import distarray
from ..array import extent as ext
from ..array.blocks import gather_slabs, slabs, whole, with_tiles
from .base import Expr, as_array

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
METRICS = ('sqeuclidean', 'euclidean', 'manhattan', 'rbf')


class PairwiseKernelExpr(Expr):
  _members = ('x', 'y')

  def compute_shape(self):
    return (self.x.shape[0], self.y.shape[0])

  def compute_dtype(self):
    return np.dtype(self.x.dtype)

  def pretty_str(self):
    return 'PairwiseKernel[%d](%s, %s, %s, gamma=%r)' % (self.expr_id, self.x, self.y, self.metric, self.gamma)

  def _evaluate(self, deps):
    # (``same``: Y was not given, y is x)
    return pairwise_array(distarray.as_array(deps['x']), None if self.same else distarray.as_array(deps['y']),
                          self.metric, self.gamma)


class AffinityPair:
  """The value of a ``NormalizedAffinityExpr``: the arrays L (n, n) and D (n)."""

  def __init__(self, L, D):
    self.parts = (L, D)
    self.shape, self.dtype = tuple(L.shape), np.dtype(L.dtype)


class NormalizedAffinityExpr(Expr):
  _members = ('x',)

  def compute_shape(self):
    return (self.x.shape[0], self.x.shape[0])

  def compute_dtype(self):
    return np.dtype(self.x.dtype)

  def pretty_str(self):
    return 'NormalizedAffinity[%d](%s, %s, gamma=%r, diagonal=%r)' % (self.expr_id, self.x, self.metric, self.gamma,
                                                                       self.diagonal)

  def _evaluate(self, deps):
    return AffinityPair(*affinity_arrays(distarray.as_array(deps['x']), self.metric, self.gamma, self.diagonal))


class AffinityPartExpr(Expr):
  """L (``part`` 0) or D (1) of a ``NormalizedAffinityExpr``."""
  _members = ('pair',)

  def compute_shape(self):
    n = self.pair.shape[0]
    return (n, n) if self.part == 0 else (n,)

  def compute_dtype(self):
    return np.dtype(self.pair.dtype)

  def pretty_str(self):
    return '%s(%s)' % (('L', 'D')[self.part], self.pair)

  def _evaluate(self, deps):
    return deps['pair'].parts[self.part]


def _points(who, name, a):
  from .sparse import is_sparse
  if is_sparse(a):
    raise TypeError('%s: %s is a sparse array, which is not accepted here: convert it with todense() first'
                    % (who, name))
  a = as_array(a)
  if len(a.shape) != 2:
    raise ValueError('%s: %s must be 2-d (points, features), got shape %s' % (who, name, tuple(a.shape)))
  if a.shape[1] < 1:
    raise ValueError('%s: %s has no features (shape %s)' % (who, name, tuple(a.shape)))
  if np.dtype(a.dtype) not in _FLOATS:
    raise ValueError('%s: %s has dtype %s; float32 / float64 are served: convert it with astype'
                     % (who, name, np.dtype(a.dtype)))
  return a


def _metric(who, metric, gamma):
  if metric == 'scaled_euclidean':
    raise ValueError("%s: metric 'scaled_euclidean' is not built (the reference's function of that name ignores the "
                     'difference of its two points); the metrics are %s' % (who, ', '.join(METRICS)))
  if metric not in METRICS:
    raise ValueError('%s: unknown metric %r; the metrics are %s' % (who, metric, ', '.join(METRICS)))
  gamma = float(gamma)
  if not (gamma >= 0.0 and np.isfinite(gamma)):
    raise ValueError('%s: gamma = %r is not finite and >= 0' % (who, gamma))
  return gamma


def pairwise_kernel(X, Y=None, metric='rbf', gamma=1.0):
  """The (n, m) matrix of ``metric`` between the rows of ``X`` (n, d) and of
  ``Y`` (m, d; None: X itself), lazily, in the inputs' one float32 / float64
  dtype: 'sqeuclidean' s_ij = sum_k (x_ik - y_jk)^2, 'euclidean' sqrt(s_ij),
  'manhattan' sum_k |x_ik - y_jk|, 'rbf' exp(-gamma s_ij) (``gamma`` is read by
  rbf only).  Equal rows give exactly 0 (rbf: 1); with Y None the result is
  bitwise symmetric.  Tiled in row slabs at X's row cuts.  A NaN coordinate
  makes that point's row (column) NaN and nothing else."""
  who = 'pairwise_kernel'
  X = _points(who, 'X', X)
  if Y is not None:
    Y = _points(who, 'Y', Y)
    if Y.shape[1] != X.shape[1]:
      raise ValueError('%s: X has %d features and Y has %d' % (who, X.shape[1], Y.shape[1]))
    if np.dtype(Y.dtype) != np.dtype(X.dtype):
      raise ValueError('%s: X and Y must have one dtype, got %s and %s: convert with astype'
                       % (who, np.dtype(X.dtype), np.dtype(Y.dtype)))
  gamma = _metric(who, metric, gamma)
  node = PairwiseKernelExpr(x=X, y=X if Y is None else Y)
  node.metric, node.gamma, node.same = metric, gamma, Y is None
  return node


def normalized_affinity(X, metric='rbf', gamma=1.0, diagonal=1.0):
  """``(L, D)``, lazily, of the (n, d) float32 / float64 points ``X``: with
  a_ij the ``metric`` of rows i and j (see ``pairwise_kernel``), the degrees
  D_i = sum_j a_ij, shape (n,), and L_ij = a_ij / sqrt(D_i D_j), shape (n, n),
  with every diagonal element set to ``diagonal``; a degree of 0 scales by 1.
  L is bitwise symmetric.  The two share one evaluation (two kernel launches a
  row slab); the unscaled matrix is never stored."""
  who = 'normalized_affinity'
  X = _points(who, 'X', X)
  gamma = _metric(who, metric, gamma)
  diagonal = float(diagonal)
  if np.isnan(diagonal):
    raise ValueError('%s: diagonal is NaN' % who)
  node = NormalizedAffinityExpr(x=X)
  node.metric, node.gamma, node.diagonal = metric, gamma, diagonal
  parts = []
  for part in (0, 1):
    e = AffinityPartExpr(pair=node)
    e.part = part
    parts.append(e)
  return tuple(parts)


# ------------------------------------------------------------- evaluation
def _row_slabs(x):
  """[(lo, hi, worker)] of x cut at its row cuts, each on the owner of its first tile."""
  return [(e.ul[0], e.lr[0], w) for e, w in slabs(x, 0)]


def pairwise_array(x, y, metric, gamma):
  """The (n, m) array of the dense 2-d arrays x and y (None: x).  Collective."""
  ctx = runtime.get()
  be = backend.get()
  x = with_tiles(x)
  y = x if y is None else with_tiles(y)
  n, m = int(x.shape[0]), int(y.shape[0])
  ys = whole(y)  # the partner points: all of them on every rank
  if x.replicated:
    return distarray.ReplicatedArray(be.pairwise(be.contiguous(x.device_data()), ys, metric, gamma, out=True)[0])
  sl = _row_slabs(x)
  tiles = {ext.create((lo, 0), (hi, m), (n, m)): w for lo, hi, w in sl}
  if y is x:  # the rows of a slab are slices of what is at hand
    blocks = {i: ys[lo:hi] for i, (lo, hi, w) in enumerate(sl) if ctx.is_local(w)}
  else:
    blocks = gather_slabs(x, 0)[1]
  local = {}
  for i, (lo, hi, w) in enumerate(sl):
    if ctx.is_local(w):
      local[ext.create((lo, 0), (hi, m), (n, m))] = be.pairwise(be.contiguous(blocks[i]), ys, metric, gamma,
                                                                out=True)[0]
  return distarray.from_tiles((n, m), x.dtype, tiles, local)


def _inv_sqrt(deg, tdt):
  """1 / sqrt(deg) in float64, 1 where deg == 0, as ``tdt`` (n values: plumbing)."""
  import torch
  d = deg.to(torch.float64)
  return torch.where(d == 0, torch.ones_like(d), d.sqrt().reciprocal()).to(tdt).contiguous()


def affinity_arrays(x, metric, gamma, diagonal):
  """The arrays (L, D) of the dense 2-d array x.  Collective."""
  ctx = runtime.get()
  be = backend.get()
  x = with_tiles(x)
  n = int(x.shape[0])
  xs = whole(x)
  if x.replicated:
    deg = be.pairwise(xs, xs, metric, gamma, row_sums=True)[1]
    sc = _inv_sqrt(deg, xs.dtype)
    L = be.pairwise(xs, xs, metric, gamma, out=True, row_scale=sc, col_scale=sc, diag_col0=0, diag_value=diagonal)[0]
    return distarray.ReplicatedArray(L), distarray.ReplicatedArray(deg)
  sl = _row_slabs(x)
  mine = [(lo, hi) for lo, hi, w in sl if ctx.is_local(w)]
  dtiles = {ext.create((lo,), (hi,), (n,)): w for lo, hi, w in sl}
  dlocal = {ext.create((lo,), (hi,), (n,)): be.pairwise(xs[lo:hi], xs, metric, gamma, row_sums=True)[1]
            for lo, hi in mine}
  D = distarray.from_tiles((n,), x.dtype, dtiles, dlocal)
  sc = _inv_sqrt(whole(D), xs.dtype)  # every degree on every rank
  ltiles = {ext.create((lo, 0), (hi, n), (n, n)): w for lo, hi, w in sl}
  llocal = {}
  for lo, hi in mine:
    llocal[ext.create((lo, 0), (hi, n), (n, n))] = be.pairwise(xs[lo:hi], xs, metric, gamma, out=True,
                                                               row_scale=sc[lo:hi].contiguous(), col_scale=sc,
                                                               diag_col0=lo, diag_value=diagonal)[0]
  return distarray.from_tiles((n, n), x.dtype, ltiles, llocal), D

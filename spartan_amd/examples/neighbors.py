"""The reference's unsupervised nearest-neighbour learner on the MI355X path
(spartan/examples/sklearn/neighbors/unsupervised.py): ``NearestNeighbors(
n_neighbors, algorithm).fit(X).kneighbors(Q)`` -> ``(dist, ind)`` host arrays.

The reference's brute path broadcasts to (Q, N, D), reduces to a (Q, N)
distance matrix and sorts the whole matrix twice; its tree paths run
scikit-learn per tile and merge on the master.  Here every ``algorithm`` value
runs the same exact search and the (Q, N) matrix is never formed:

  * Q is replicated as fp64; X is cut into whole-row blocks as k-means cuts it;
  * each owner runs ``backend.knn`` (spx_knn: distances and selection fused) on
    its blocks with ``index_base`` = the block's first row, giving per block
    the ``min(k, rows)`` best (s, index) per query, s the exact-order fp64 sum
    of squared differences;
  * the blocks' lists are gathered in row order and concatenated along axis 1
    (position order is then index order for equal s) and reduced with
    ``backend.topk(..., in_idx=...)``;
  * ``dist = sqrt(s)`` rounded once to X's dtype, on the GPU.

One block on one rank takes no exchange and no combine.

Contract: neighbours are the first k of the order (s, index);
``dist[i, r]`` carries the bits of the exact-order cdist entry (i, ind[i, r]).
Selection is on s, not on the rounded distance.  The reference sorts the
array-dtype values of a NumPy tile sum instead, so where two distances round to
the same float32 its order between them may differ; that is not restated.
"""
import numpy as np

from .. import backend, expr, runtime
from ..array import distarray, extent as ext
from .kmeans import _replicated_f64, _row_blocks

ALGORITHMS = ('auto', 'ball_tree', 'kd_tree', 'brute')


def _forced(a):
  if isinstance(a, np.ndarray):
    a = expr.from_numpy(a)
  return distarray.as_array(expr.force(a))


class NearestNeighbors(object):
  """Unsupervised learner for neighbour searches (the reference's signature).
  All four ``algorithm`` values run the same exact search."""

  def __init__(self, n_neighbors=5, algorithm='auto'):
    if algorithm not in ALGORITHMS:
      raise ValueError('NearestNeighbors: algorithm %r is not one of %s' % (algorithm, ALGORITHMS))
    self.n_neighbors = n_neighbors
    self.algorithm = algorithm

  def fit(self, X):
    if isinstance(X, np.ndarray):
      X = expr.from_numpy(X)
    if len(X.shape) != 2:
      raise ValueError('NearestNeighbors.fit: X must be 2-d, got shape %s' % (tuple(X.shape),))
    self.X = X
    return self

  def kneighbors(self, X, n_neighbors=None):
    """(dist, ind): for each row of ``X`` the ``n_neighbors`` nearest rows of
    the fitted data, nearest first, ties by index; dist in the fitted data's
    dtype, ind int64."""
    if n_neighbors is not None:
      self.n_neighbors = n_neighbors
    k = self.n_neighbors
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
      raise ValueError('NearestNeighbors: n_neighbors %r must be a positive integer' % (k,))
    k = int(k)
    pts = _forced(self.X)
    qry = _forced(X)
    if len(qry.shape) != 2 or qry.shape[1] != pts.shape[1]:
      raise ValueError('NearestNeighbors.kneighbors: queries of shape %s against data of shape %s'
                       % (tuple(qry.shape), tuple(pts.shape)))
    N = pts.shape[0]
    if k > N:
      raise ValueError('NearestNeighbors: n_neighbors %d exceeds the %d fitted points' % (k, N))
    if k > backend.KNN_K_MAX:
      raise ValueError('NearestNeighbors: n_neighbors %d exceeds KNN_K_MAX = %d' % (k, backend.KNN_K_MAX))
    dt = np.dtype(pts.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
      raise ValueError('NearestNeighbors: data must be float32 / float64, not %s' % dt)
    s, ind = kneighbors_arrays(pts, qry, k)
    # sqrt and the one rounding to X's dtype as a generated map over the (Q, k)
    # sums (held by every rank): the device sqrt k_cdist calls
    dist = expr.astype(expr.sqrt(expr.lazify(distarray.ReplicatedArray(s))), dt).glom()
    return dist, ind.cpu().numpy()


def _knn_block(be, pts, q, k, base):
  import torch
  kb = min(k, int(pts.shape[0]))
  s = torch.empty((q.shape[0], kb), dtype=torch.float64, device=q.device)
  ind = torch.empty((q.shape[0], kb), dtype=torch.int64, device=q.device)
  be.knn(pts, q, kb, base, s, ind)
  return s, ind


def kneighbors_arrays(pts, qry, k):
  """(s, ind) device tensors (Q, k), the same on every rank (collective)."""
  import torch
  ctx = runtime.get()
  be = backend.get()
  Q, D = qry.shape
  if getattr(qry, 'replicated', False):
    q = be.contiguous(qry.device_data(), np.float64)
  else:
    q = _replicated_f64(qry)
  if getattr(pts, 'replicated', False):  # held in full by every rank: no exchange
    return _knn_block(be, be.contiguous(pts.device_data()), q, k, 0)
  blocks, got = _row_blocks(pts, D)
  if len(blocks) == 1 and ctx.world_size == 1:
    return _knn_block(be, got[0], q, k, 0)
  # the blocks' lists as the column tiles of one (Q, total) array, in row order
  widths = [min(k, r.lr[0] - r.ul[0]) for _src, r in blocks]
  total = sum(widths)
  tiles, loc_s, loc_i = {}, {}, {}
  off = 0
  for qi, (src, region) in enumerate(blocks):
    e = ext.create((0, off), (Q, off + widths[qi]), (Q, total))
    off += widths[qi]
    tiles[e] = src  # worker id == owner rank
    if src == ctx.rank:
      loc_s[e], loc_i[e] = _knn_block(be, got[qi], q, k, region.ul[0])
  if Q == 0:
    return (torch.empty((0, k), dtype=torch.float64, device=ctx.device),
            torch.empty((0, k), dtype=torch.int64, device=ctx.device))
  all_s = distarray.from_tiles((Q, total), np.dtype(np.float64), tiles, loc_s)
  all_i = distarray.from_tiles((Q, total), np.dtype(np.int64), tiles, loc_i)
  full = ext.from_shape((Q, total))
  everyone = [(full, r) for r in range(ctx.world_size)]
  cs = be.contiguous(distarray.gather_regions(all_s, everyone)[ctx.rank])
  ci = be.contiguous(distarray.gather_regions(all_i, everyone)[ctx.rank])
  s = torch.empty((Q, k), dtype=torch.float64, device=cs.device)
  ind = torch.empty((Q, k), dtype=torch.int64, device=cs.device)
  be.topk(cs, ci, s, ind, (Q, total, 1), k, False)
  return s, ind

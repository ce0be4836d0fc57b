"""PageRank power iteration on a sparse link matrix.

The reference's scaling benchmark (tests/test_pagerank.py there) builds a
random "site graph" -- every page has ``num_outlinks`` links, each with
probability ``same_site_prob`` to a page of its own site and else to any page
-- and multiplies the link matrix into the rank vector ``num_iter`` times.
Here the sites are contiguous blocks of ceil(sqrt(num_pages)) pages (the
reference uses one block per worker, which would tie the data to the layout),
the matrix is column-normalised (column j holds 1 / num_outlinks per link of
page j, repeated links summed) and the iteration is the damped one:

    p <- damping * W p + (1 - damping) / n
"""
import numpy as np

from .. import expr
from ..array import sparse as sparray
from ..expr.sparse import SparseVal


def site_graph(num_pages, num_outlinks, same_site_prob, seed, tile_hint=None):
  """The (num_pages, num_pages) float32 link matrix as a sparse expression:
  W[i, j] = (links from page j to page i) / num_outlinks.  Every rank draws the
  whole graph from ``np.random.RandomState(seed)`` on the host and keeps its
  row slabs (ingest): the matrix depends on the seed alone."""
  import scipy.sparse as sp
  n, k = int(num_pages), int(num_outlinks)
  rs = np.random.RandomState(seed)
  site = max(1, int(np.ceil(np.sqrt(n))))
  page = np.repeat(np.arange(n, dtype=np.int64), k)
  lo = (page // site) * site
  hi = np.minimum(lo + site, n)
  same = rs.random_sample(n * k) <= same_site_prob
  inside = lo + (rs.random_sample(n * k) * (hi - lo)).astype(np.int64)
  anywhere = rs.randint(0, n, n * k)
  target = np.where(same, inside, anywhere)
  vals = np.full(n * k, 1.0 / k, np.float32)
  W = sp.coo_matrix((vals, (target, page)), shape=(n, n), dtype=np.float32)
  return SparseVal(val=sparray.from_scipy(W, tile_hint))


def pagerank(W, damping=0.85, num_iter=5):
  """``num_iter`` damped power iterations from the uniform vector; returns the
  (n, 1) rank vector as a forced expression.  ``W`` is sparse or dense."""
  W = expr.as_array(W)
  n = W.shape[1]
  dt = np.dtype(W.dtype)
  p = expr.eager(expr.ones((n, 1), dtype=dt) * dt.type(1.0 / n))
  for _ in range(num_iter):
    p = expr.eager(expr.dot(W, p) * dt.type(damping) + dt.type((1.0 - damping) / n))
  return p

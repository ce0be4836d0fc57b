"""The reference's fuzzy k-means driver (spartan/examples/fuzzy_kmeans.py) on
the fused soft-assignment step (``expr.fuzzy_assign``).

The reference builds an (n, k, d) broadcast for the distances, an (n, k, k)
broadcast for the memberships and a second (n, k, d) broadcast for the weighted
sums, every iteration.  Here an iteration is one pass over the points: the
labels, the membership totals and the membership-weighted sums come out of
one kernel launch per row slab, and only the (k,) totals and the (k, d) sums
travel to the host, as in the reference's ``glom()``.

Divergences from the reference, kept on purpose:

  * THE MEMBERSHIP RULE.  The reference's live expression divides
    ``reshape(distances, (n, 1, k))`` by ``reshape(distances, (n, k, 1))`` and
    sums over the last axis, which gives ``prob_i = d_i^e / sum_j d_j^e``: the
    membership grows with the distance and ``argmax(prob)`` labels every point
    with its FARTHEST centre.  The routine the reference keeps in its
    docstring (``_calc_probability``: ``1 / sum_j (d_i / d_j)^e``) is the
    intended rule -- the nearest centre has the largest membership -- and is
    the one built here;
  * centres that receive no membership are reseeded from a generator seeded by
    ``seed`` instead of the global ``np.random`` (as ``examples.kmeans`` does);
  * ``weight_power``: 1.0 weighs a point by its membership u, the reference's
    update; ``weight_power=m`` weighs it by u^m, the textbook fuzzy c-means.

Not built: a convergence test or an objective value, K above the kernel's
``kmax``, sparse points, distributed centres.
"""
import numpy as np

from .. import expr


def fuzzy_kmeans(points, k=10, num_iter=10, m=2.0, centers=None, seed=0, weight_power=1.0, return_centers=False):
  """Cluster the (n, d) float32 / float64 ``points`` into ``k`` fuzzy clusters
  by ``num_iter`` iterations with fuzzifier ``m`` (> 1).  ``centers``: the
  (k, d) start (host array, array or expression), or None for ``expr.rand``.
  Returns the labels of the last iteration (a lazy (n,) int64 expression: the
  nearest centre of every point), or ``(labels, centers)`` -- the final (k, d)
  float64 host array -- with ``return_centers``."""
  if isinstance(points, np.ndarray):
    points = expr.from_numpy(points)
  points = expr.lazify(expr.as_array(points).force())  # evaluated once, not once an iteration
  num_dim = points.shape[1]
  rng = np.random.default_rng(seed)
  if centers is None:
    centers = expr.rand(k, num_dim)
  centers = np.asarray(expr.as_array(centers).glom(), dtype=np.float64)
  if centers.shape != (k, num_dim):
    raise ValueError('fuzzy_kmeans: the centres must be (%d, %d), got shape %s' % (k, num_dim, centers.shape))
  labels = expr.zeros((points.shape[0],), dtype=np.int64)
  for _ in range(num_iter):
    labels, counts, sums = expr.fuzzy_assign(points, centers, m=m, weight_power=weight_power)
    counts = np.array(counts.glom(), dtype=np.float64)
    sums = np.array(sums.glom(), dtype=np.float64)
    empty = counts == 0
    if np.any(empty):
      counts[empty] = 1
      sums[empty, :] = rng.random((int(np.count_nonzero(empty)), num_dim))
    centers = sums / counts[:, None]
  return (labels, centers) if return_centers else labels

"""The reference's spectral clustering (spartan/examples/spectral_clustering.py)
on the pairwise kernel (``expr.normalized_affinity``).

The reference writes the two matrix-building steps as ``shuffle`` calls: a
Python double loop over pairs of points for the affinity matrix A, then a
second pass that scales A to D^-1/2 A D^-1/2 and sets a unit diagonal.  Here
both are ``normalized_affinity``: two launches of one kernel per row slab, and
A itself is never stored.  The rest of the chain is the reference's, line by
line, on what the project already has:

    L       = D^-1/2 A D^-1/2 with a unit diagonal
    d, U    = lanczos.solve(L, L, min(2 k, n), True)
    U       = U[:, :k]
    centres = U[argmax(U, axis=0)]      one row per column: where it is largest
    labels  = KMeans(k, num_iter).fit(U, centres)

Divergences from the reference, kept on purpose:

  * 'scaled_euclidean' is refused.  The reference's
    ``scaled_euclidean_distance`` calls ``np.square(X, Y)``, which squares X
    INTO Y and ignores the difference of the two points (and overwrites the
    second point on the way); the rule of its docstring needs the median over
    the features of every pair's squared differences, a different kernel.
    tests/test_affinity.py pins the disagreement;
  * 'sqeuclidean' is accepted beside the reference's 'manhattan', 'euclidean'
    and 'rbf'.

Not built: a Lanczos step fused into the pair kernel (L is stored, (n, n)); a
point set too large for one GPU to hold whole.
"""
import numpy as np

from .. import expr
from . import lanczos
from .kmeans import KMeans


def spectral_cluster(points, k=10, num_iter=10, similarity_measurement='rbf'):
  """Cluster the (n, d) ``points`` into ``k`` groups by k-means on the leading
  eigenvectors of the normalised affinity matrix.

  Args:
    points: array or expression of shape (n, d), float32 / float64.
    k(int): the number of clusters.
    num_iter(int): the k-means iterations.
    similarity_measurement(str): 'rbf' (gamma 1), 'euclidean', 'manhattan' or 'sqeuclidean'.

  Returns:
    the labels, as ``KMeans.fit`` returns them.
  """
  n = points.shape[0]
  L, _D = expr.normalized_affinity(points, metric=similarity_measurement, gamma=1.0, diagonal=1.0)
  L = expr.lazify(expr.as_array(L).force())  # evaluated once: every Lanczos step multiplies by it
  overshoot = min(k * 2, n)
  _d, U = lanczos.solve(L, L, overshoot, True)
  U = np.ascontiguousarray(U[:, 0:k])
  init_clusters = U[np.argmax(U, axis=0)]
  _centers, labels = KMeans(k, num_iter).fit(expr.from_numpy(U), init_clusters)
  return labels

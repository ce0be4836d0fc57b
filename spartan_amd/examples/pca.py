"""The reference's ``spartan/examples/pca.py`` on the MI355X path: the class
``PCA`` (pca.py:6-71) restated on ``examples.ssvd.svd``, whose orthogonal
factor comes from the Householder TSQR of ``expr.qr``."""
import numpy as np

from .. import expr
from ..array import distarray
from .ssvd import svd


class PCA(object):
  """Principal component analysis (PCA) on the stochastic SVD."""

  def __init__(self, n_components=None):
    self.n_components = n_components

  def fit(self, X, rank=None):
    """Fit the model to the data X (pca.py:16-40).

    Args:
      X: array or expression of shape (n_samples, n_features).
      rank(int): the rank of this matrix (default min(n_samples, n_features)).

    Returns:
      self
    """
    X = expr.as_array(X)
    self.mean_ = expr.mean(X, axis=0)
    X = X - self.mean_
    if rank is None:
      rank = min(X.shape[0], X.shape[1])
    V, S, U = svd(X, rank)
    self.components_ = U
    self.components_ = self.components_[:self.n_components, :]
    return self

  def transform(self, X):
    """Reduce dimensions of matrix X (pca.py:42-55): a NumPy array of shape
    (n_samples, n_components)."""
    X_transformed = expr.as_array(X) - self.mean_
    return expr.dot(X_transformed, np.ascontiguousarray(self.components_.T)).optimized().glom()

  def inverse_transform(self, X):
    """Transform data back to its original space (pca.py:57-71): an array for
    an expression or a distributed array, else a NumPy array of shape
    (n_samples, n_features)."""
    if isinstance(X, (expr.Expr, distarray.DistArray)):
      return (expr.dot(X, self.components_) + self.mean_).optimized().force()
    return np.dot(X, self.components_) + self.mean_.glom()

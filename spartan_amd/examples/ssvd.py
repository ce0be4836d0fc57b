"""The reference's ``spartan/examples/ssvd`` package (``qr.py`` and ``ssvd.py``)
on the MI355X path.

``qr(Y)`` restates ``ssvd/qr.py:7-48``: the same signature and return types (Q
a distributed array of shape (M, K), R a NumPy array of shape (K, K)).  The
reference forms Y'Y, a host Cholesky factor and its inverse (CholeskyQR, which
loses orthogonality as cond(Y)^2 u); here the pair comes from ``expr.qr`` -- a
Householder TSQR on spx_geqr / spx_orgqr, stable for any conditioning, with
diag(R) >= 0 (expr/qr.py).

``svd(A, k)`` restates ``ssvd/ssvd.py:6-49`` line by line.  One deliberate
deviation: the k x k eigenproblem of B B' uses ``np.linalg.eigh`` on the
symmetrised matrix; the reference's ``np.linalg.eig`` may return complex pairs
for a matrix that is symmetric only up to rounding."""
import numpy as np

from .. import expr


def qr(Y):
  """Compute the thin qr factorization of a matrix: Y = Q R, Q orthonormal and
  R upper-triangular.

  Args:
    Y: array or expression of shape (M, K), M >= K.

  Returns:
    Q: distributed array of shape (M, K).
    R: NumPy array of shape (K, K).
  """
  Q, R = expr.qr(Y)
  return Q.force(), R.glom()


def svd(A, k=None):
  """Stochastic SVD.

  Args:
    A: array or expression of shape (M, N).
    k(int): number of singular values and vectors to compute (default N).

  Returns:
    U: distributed array of shape (M, k)
    S: NumPy array of shape (k,)
    V: NumPy array of shape (k, N)
  """
  A = expr.as_array(A)
  if k is None:
    k = A.shape[1]
  Omega = expr.randn(A.shape[1], k, dtype=A.dtype)
  Y = expr.dot(A, Omega)
  Q, R = qr(Y)
  Q = expr.lazify(Q)
  B = expr.dot(expr.transpose(Q), A).optimized().glom()
  BBT = B.dot(B.T)
  S, U_ = np.linalg.eigh((BBT + BBT.T) / 2)
  S = np.sqrt(S)
  # Sort by eigen values from large to small
  si = np.argsort(S)[::-1]
  S = S[si]
  U_ = U_[:, si]
  U = expr.dot(Q, U_).optimized().force()
  V = np.dot(np.dot(B.T, U_), np.diag(np.ones(S.shape[0], B.dtype) / S))
  return U, S, V.T

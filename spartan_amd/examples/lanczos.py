"""The reference's ``spartan/examples/lanczos.py`` on the MI355X path.

``solve(A, AT, desired_rank, is_symmetric)`` restates the reference's
function: the same signature, the same return types (NumPy arrays) and the
same iteration line by line -- only the matrix * vector step is distributed,
the Lanczos vectors stay on the host, every new vector is re-orthogonalised
against all earlier ones.  One deliberate deviation, the one
``examples/ssvd.py`` documents for its own eigenproblem: the
(desired_rank + 2)-square tridiagonal matrix is symmetric, so its eigenpairs
come from ``expr.eigh`` on the device (the Jacobi kernel behind spx_syevj)
instead of the host's ``np.linalg.eig``, which may return complex pairs for a
matrix that is symmetric only up to rounding.

The operands are dense arrays or expressions: a sparse ``A`` still stops at
``transpose`` and at the dense ``dot`` of a column vector's result, as
everywhere else (convert it with ``todense()`` first)."""
import numpy as np

from .. import expr


def solve(A, AT, desired_rank, is_symmetric=False):
  """The ``desired_rank`` eigenvalues of largest magnitude of AT A (of A where
  ``is_symmetric``) and their eigenvectors, by the Lanczos iteration.

  Args:
    A: array or expression of shape (M, N).
    AT: its transpose (not used where ``is_symmetric``).
    desired_rank(int): number of eigenpairs.
    is_symmetric(bool): iterate with A itself.

  Returns:
    d: NumPy array of shape (desired_rank,), by decreasing magnitude.
    s: NumPy array of shape (N, desired_rank), the eigenvectors as columns.
  """
  # two more steps than asked for, dropped at the end (this keeps the result in line with scipy.sparse.linalg.svds)
  desired_rank += 2

  n = A.shape[1]
  v_next = np.ones(n) / np.sqrt(n)
  v_prev = np.zeros(n)
  beta = np.zeros(desired_rank + 1)
  alpha = np.zeros(desired_rank)
  V = np.zeros((n, desired_rank))  # the Lanczos vectors: desired_rank << n, kept on the host

  for i in range(desired_rank):
    v_next_expr = expr.from_numpy(v_next.reshape(n, 1))
    if is_symmetric:
      w = expr.dot(A, v_next_expr).optimized().glom().reshape(n)
    else:
      w = expr.dot(A, v_next_expr)
      w = expr.dot(AT, w).optimized().glom().reshape(n)

    alpha[i] = np.dot(w, v_next)
    w = w - alpha[i] * v_next - beta[i] * v_prev

    for t in range(i):  # full re-orthogonalisation
      tmpa = np.dot(w, V[:, t])
      if tmpa == 0.0:
        continue
      w -= tmpa * V[:, t]

    beta[i + 1] = np.linalg.norm(w, 2)
    v_prev = v_next
    v_next = w / beta[i + 1]
    V[:, i] = v_prev

  tridiag = np.diag(alpha)
  for i in range(desired_rank - 1):
    tridiag[i, i + 1] = beta[i + 1]
    tridiag[i + 1, i] = beta[i + 1]

  # the eigenvalues of the tridiagonal matrix are those of AT A; V times its eigenvectors gives AT A's
  d, v = expr.eigh(tridiag)
  d, v = d.glom(), v.glom()

  sorted_idx = np.argsort(np.absolute(d))[::-1]
  d = d[sorted_idx]
  v = v[:, sorted_idx]

  s = np.dot(V, v)
  return d[0:desired_rank - 2], s[:, 0:desired_rank - 2]

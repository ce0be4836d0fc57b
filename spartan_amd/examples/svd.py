"""The reference's ``spartan/examples/svd.py`` on the MI355X path: ``svds(A, k)``
restates its function -- two Lanczos solves (``examples/lanczos.py``), one for
the left and one for the right singular vectors -- with the same signature and
return types.  ``A`` is a dense array or expression: a sparse one still stops
at ``transpose``, as everywhere else (convert it with ``todense()`` first)."""
import numpy as np

from .. import expr
from . import lanczos


def svds(A, k=6):
  """Compute the largest k singular values / vectors of a matrix.

  Args:
    A: array or expression of shape (M, N).
    k(int): number of singular values and vectors to compute.

  Returns:
    u: NumPy array of shape (M, k), the left singular vectors as columns.
    s: NumPy array of shape (k,), the singular values.
    vt: NumPy array of shape (k, N), the right singular vectors as rows.
  """
  A = expr.as_array(A)
  AT = expr.transpose(A)
  d, u = lanczos.solve(AT, A, k)
  d, v = lanczos.solve(A, AT, k)
  return u, np.sqrt(d), v.T

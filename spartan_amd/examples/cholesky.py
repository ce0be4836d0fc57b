"""The reference's ``spartan/examples/cholesky.py`` on the MI355X path:
``cholesky(A)`` returns the expression of the lower factor with zeros above
the diagonal.

The reference forces ``A``, assumes ``sqrt(len(A.tiles))`` equal square tiles
and runs its right-looking loop with scipy's dpotrf / dtrtrs / dsyrk / dgemm
per tile.  ``expr.cholesky`` runs that loop on spx_potrf / spx_trsm / spx_syrk
for such a grid and accepts every other layout as well (expr/linalg.py)."""
from .. import expr


def cholesky(A):
  """Cholesky matrix decomposition.

  Args:
    A(Expr): matrix to be decomposed (symmetric positive definite; the lower
      triangle is read)
  """
  return expr.cholesky(A)

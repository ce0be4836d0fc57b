"""Conjugate gradient and the NAS-CG outer iteration (the
reference's spartan/examples/conj_gradient.py has the same two signatures).

``cgit(A, x)`` runs 15 steps of the conjugate-gradient method for A z = x from
z = 0 (A symmetric positive definite, sparse or dense; x of shape (n, 1) or
(n,)).  ``conj_gradient(A, num_iter)`` is the inverse power iteration of the
NAS CG benchmark (RNR-94-007, p. 19-20): x <- z / ||z|| with z = cgit(A, x).

The three scalars of a step (rho, p.q, the new rho) come to the host, as in the
reference; every vector stays on the device in A's row slabs.
"""
from .. import expr

CG_STEPS = 15


def _scalar(e):
  return float(e.glom())


def cgit(A, x, steps=CG_STEPS):
  """An approximate solution z of A z = x after ``steps`` CG steps."""
  A = expr.as_array(A)
  x = expr.as_array(x)
  r = expr.eager(x)
  z = None
  p = r
  rho = _scalar(expr.sum(r * r))
  for _ in range(steps):
    if rho == 0.0:  # the residual vanished: z is exact
      break
    q = expr.eager(expr.dot(A, p))
    alpha = rho / _scalar(expr.sum(p * q))
    z = expr.eager(p * alpha if z is None else z + p * alpha)
    r = expr.eager(r - q * alpha)
    rho0, rho = rho, _scalar(expr.sum(r * r))
    p = expr.eager(r + p * (rho / rho0))
  return z if z is not None else expr.eager(x * 0.0)


def conj_gradient(A, num_iter=15):
  """``num_iter`` rounds of x <- z / ||z||, z = cgit(A, x), from the ones
  vector; returns the unit vector x (n, 1)."""
  A = expr.as_array(A)
  x = expr.eager(expr.ones((A.shape[1], 1), dtype=A.dtype))
  for _ in range(num_iter):
    z = cgit(A, x)
    x = expr.eager(z / _scalar(expr.norm(z)))
  return x

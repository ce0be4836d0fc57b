"""Alternating least squares on a sparse rating matrix (the
reference's spartan/examples/als.py, the driver of its Netflix example).

``A`` (users x items) is factored as U M^T.  A half-step holds one factor fixed
and solves, for every row of the rating matrix (or of its transpose), the
regularised normal equations over the row's nonzero ratings,

    (sum_k y_k y_k^T + la |K_i| I) x_i = sum_k a_ik y_k,

which the reference does in a Python loop with one ``lstsq`` per row and this
build in one kernel launch per slab (``spx_als_solve``).  The transpose is built
once, by ``sparse_transpose``.
"""
import numpy as np

from .. import backend, comm, expr, runtime
from ..array import sparse as sparray
from ..expr import sparse as spexpr
from ..expr.builtins import _new_seed


def half_step(S, Y, la):
  """(X, infos): the rows of the sparse ``S`` solved against the dense factor
  ``Y`` -- X a forced dense expression in S's row slabs, ``infos`` the unread
  device counters of failed rows (``expr.sparse.sparse_als_solve``)."""
  Sa = spexpr.as_sparse_expr(S).force()
  X, infos = spexpr.sparse_als_solve(Sa, expr.as_array(Y).force(), float(la))
  return expr.lazify(X), infos


def _initial_items(AT, num_features, seed):
  """The reference's starting M: uniform random numbers, column 0 overwritten
  with every item's average rating -- sum / count over the nonzero stored
  entries of its row of ``AT`` -- and 0 for an item nobody rated."""
  import torch
  from .. import codegen
  be = backend.get()
  n, m = AT.shape
  dt = np.dtype(AT.dtype)
  indicator = codegen.Cast(codegen.Op('not_equal', [codegen.In(0, dt), codegen.Sc(0, 0.0)]), dt)

  def rated(v):
    out = torch.empty_like(v)
    if v.numel():
      be.map(indicator, {0: v}, out)
    return out

  ones = np.ones(m, dtype=dt)
  total = expr.dot(spexpr.SparseVal(val=AT), ones)
  count = expr.dot(spexpr.SparseVal(val=AT.with_values(rated)), ones)
  avg = total / expr.maximum(count, dt.type(1))
  M = expr.rand(n, num_features, dtype=dt, seed=_new_seed(seed))
  return expr.write(M, np.s_[:, 0:1], expr.reshape(avg, (n, 1)), np.s_[:, :]).force()


def als(A, la=0.065, alpha=40, implicit_feedback=False, num_features=20, num_iter=10, M=None, seed=None):
  """Factor the sparse rating matrix ``A`` (num_users x num_items) as U M^T by
  ``num_iter`` rounds of alternating least squares; returns (U, M) as forced
  dense expressions of A's dtype, U in A's row slabs and M in those of the
  transpose.

  ``A`` is a sparse expression, a SparseDistArray or a scipy.sparse matrix; a
  rating of exactly 0 counts as missing, as in the reference.  ``la`` > 0 is the
  regularisation (scaled by each row's number of ratings).  ``M``, when given,
  is the (num_items, num_features) starting factor -- the reference accepts the
  argument and ignores it; otherwise M starts as random numbers drawn from
  ``seed`` with the items' average ratings in column 0.  ``alpha`` belongs to
  the implicit-feedback variant, which is not built."""
  if implicit_feedback:
    raise NotImplementedError('als: implicit_feedback=True is not built (it does dense work over all items per '
                              'user: a different kernel)')
  if not spexpr.is_sparse(A):
    raise TypeError('als: a sparse rating matrix is needed, got %s: ingest a scipy.sparse matrix through '
                    'from_numpy' % type(A).__name__)
  if not (float(la) > 0 and np.isfinite(float(la))):
    raise ValueError('als: la = %r must be positive and finite: the systems must be positive definite' % (la,))
  num_features, num_iter = int(num_features), int(num_iter)
  if num_iter < 1:
    raise ValueError('als: num_iter = %d is below 1' % num_iter)
  S = spexpr.as_sparse_expr(A).force()
  fmax = backend.als_plan(S.dtype, 0)[0]
  if num_features < 1 or num_features > fmax:
    raise ValueError('als: num_features = %d is outside [1, %d], the limit of the ALS kernel' % (num_features, fmax))
  ST = sparray.transposed(S)
  if M is None:
    Mv = _initial_items(ST, num_features, seed)
  else:
    Mv = expr.as_array(M).force()
    if getattr(Mv, 'sparse', False) or tuple(Mv.shape) != (S.shape[1], num_features):
      raise ValueError('als: M must be a dense (%d, %d) array' % (S.shape[1], num_features))
  infos = []
  for _ in range(num_iter):
    Uv, i1 = spexpr.sparse_als_solve(S, Mv, float(la))
    Mv, i2 = spexpr.sparse_als_solve(ST, Uv, float(la))
    infos += i1 + i2
  _raise_if_failed(infos)
  return expr.lazify(Uv), expr.lazify(Mv)


def _raise_if_failed(infos):
  """One read of the failure counters of a whole run (collective)."""
  import torch
  ctx = runtime.get()
  bad = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
  if infos:
    bad += torch.stack([i.reshape(()) for i in infos]).sum()
  if ctx.distributed:
    comm.all_reduce(bad, 'sum')
  bad = int(bad.item())
  if bad:
    raise np.linalg.LinAlgError('als: %d row solves met a pivot that is not positive and finite' % bad)

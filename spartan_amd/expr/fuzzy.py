"""``fuzzy_assign`` / ``fuzzy_membership``: the soft assignment of fuzzy
k-means on spx_fuzzy_step.

The reference's driver (spartan/examples/fuzzy_kmeans.py) writes one iteration
as broadcasts: an (n, k, d) difference for the distances, an (n, k, k) ratio
for the memberships and a second (n, k, d) product for the weighted sums.
None of them is built here.  With ``d_j = |x - c_j|^2 + eps`` and
``e = 2 / (m - 1)`` the membership ``1 / sum_l (d_j / d_l)^e`` is

    u_j = t_j / sum_l t_l,    t_j = (d_min / d_j)^e,

every ``t_j`` in (0, 1], and the update is ``sums = W^T X``, ``counts = W^T 1``
for ``W = U^weight_power``: one pass over X, one kernel launch per row slab.

``fuzzy_assign(X, C)`` is a lazy triple ``(labels, counts, sums)`` hanging off
one node: forcing any of them runs the step once.  ``fuzzy_membership(X, C)`` is
the (n, k) matrix U itself, for the user who wants it.

Routes; every rank issues the same exchanges whether or not it owns rows:

  * C is gathered in full to every rank and held in float64;
  * a replicated X is computed whole on every rank; the results are replicated;
  * any other X is cut into row slabs at its own row cuts
    (``blocks.gather_slabs(X, 0)``: a column-cut X is gathered to row blocks by
    that one exchange); each rank runs one ``fuzzy_step`` per slab it holds,
    adding into one pair of (sums, counts) buffers, which are all-reduced once
    and delivered through ``combine.deliver``.  ``labels`` and U are tiled in
    row slabs at X's row cuts on the slabs' owners.

Divergence from the reference, kept on purpose: its live expression divides
``reshape(d, (n, 1, k))`` by ``reshape(d, (n, k, 1))``, which makes the
membership GROW with the distance (``argmax`` then names the farthest centre).
The rule built here is the one its docstring routine ``_calc_probability``
states: the nearest centre has the largest membership.

Not built: K above the kernel's ``kmax``, a sparse X, distributed centres.
"""
import numpy as np

from .. import backend, comm, runtime
from ..array import combine, distarray
from ..array import extent as ext
from ..array.blocks import deferred, gather_slabs, whole, with_tiles
from .base import Expr, as_array

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


class FuzzyTriple:
  """The value of a ``FuzzyAssignExpr``: the arrays labels, counts and sums
  (shape and dtype: the labels')."""

  def __init__(self, labels, counts, sums):
    self.parts = (labels, counts, sums)
    self.shape, self.dtype = tuple(labels.shape), np.dtype(np.int64)


class _FuzzyNode(Expr):
  _members = ('array', 'centers')

  def _args(self, deps):
    return (distarray.as_array(deps['array']), distarray.as_array(deps['centers']), self.exponent, self.eps,
            self.weight_power)


class FuzzyAssignExpr(_FuzzyNode):
  def compute_shape(self):
    return (self.array.shape[0],)

  def compute_dtype(self):
    return np.dtype(np.int64)

  def pretty_str(self):
    return 'FuzzyAssign[%d](%s, %s, exponent=%r)' % (self.expr_id, self.array, self.centers, self.exponent)

  def _evaluate(self, deps):
    return FuzzyTriple(*fuzzy_step_arrays(*self._args(deps), want_U=False))


class FuzzyPartExpr(Expr):
  """labels (``part`` 0), counts (1) or sums (2) of a ``FuzzyAssignExpr``."""
  _members = ('step',)

  def compute_shape(self):
    n, k, d = self.nkd
    return ((n,), (k,), (k, d))[self.part]

  def compute_dtype(self):
    return np.dtype(np.int64 if self.part == 0 else np.float64)

  def pretty_str(self):
    return '%s(%s)' % (('labels', 'counts', 'sums')[self.part], self.step)

  def _evaluate(self, deps):
    return deps['step'].parts[self.part]


class FuzzyMembershipExpr(_FuzzyNode):
  def compute_shape(self):
    return (self.array.shape[0], self.centers.shape[0])

  def compute_dtype(self):
    return np.dtype(self.array.dtype)

  def pretty_str(self):
    return 'FuzzyMembership[%d](%s, %s, exponent=%r)' % (self.expr_id, self.array, self.centers, self.exponent)

  def _evaluate(self, deps):
    return fuzzy_step_arrays(*self._args(deps), want_U=True)


def _checked(who, X, C, m, eps, weight_power):
  from .sparse import is_sparse
  if is_sparse(X) or is_sparse(C):
    raise TypeError('%s: a sparse array is not accepted here: convert it with todense() first' % who)
  X, C = as_array(X), as_array(C)
  if len(X.shape) != 2:
    raise ValueError('%s: a 2-d array of points is needed, got shape %s' % (who, tuple(X.shape)))
  if len(C.shape) != 2 or C.shape[1] != X.shape[1]:
    raise ValueError('%s: the centres must be (k, %d), got shape %s' % (who, X.shape[1], tuple(C.shape)))
  if C.shape[0] < 1 or X.shape[1] < 1:
    raise ValueError('%s: at least one centre and one column are needed, got %s and %s'
                     % (who, tuple(C.shape), tuple(X.shape)))
  dt = np.dtype(X.dtype)
  if dt not in _FLOATS:
    raise TypeError('%s: dtype %s is not float32 / float64' % (who, dt))
  if np.dtype(C.dtype).kind not in 'fiub':
    raise TypeError('%s: the centres\' dtype %s is not numeric' % (who, np.dtype(C.dtype)))
  m, eps, weight_power = float(m), float(eps), float(weight_power)
  if not (m > 1.0 and np.isfinite(m)):
    raise ValueError('%s: the fuzzifier m = %r must be finite and above 1' % (who, m))
  if not (eps > 0.0 and np.isfinite(eps)):
    raise ValueError('%s: eps = %r must be finite and above 0' % (who, eps))
  if not (weight_power > 0.0 and np.isfinite(weight_power)):
    raise ValueError('%s: weight_power = %r must be finite and above 0' % (who, weight_power))
  return X, C, 2.0 / (m - 1.0), eps, weight_power


def fuzzy_assign(X, C, m=2.0, eps=1e-11, weight_power=1.0):
  """``(labels, counts, sums)``, lazily, of one fuzzy k-means step of the
  (n, d) float32 / float64 points ``X`` against the (k, d) centres ``C``: with
  ``d_j = |x - c_j|^2 + eps`` and ``u_j = 1 / sum_l (d_j / d_l)^(2 / (m - 1))``,
  ``labels`` (n,) int64 is the nearest centre (the largest membership, the first
  of equals), tiled at X's row cuts; ``counts`` (k,) and ``sums`` (k, d), both
  float64, are ``sum_i u_ij^weight_power`` and ``sum_i u_ij^weight_power x_i``.
  The three share one evaluation: one pass over X, no (n, k) matrix."""
  X, C, exponent, eps, weight_power = _checked('fuzzy_assign', X, C, m, eps, weight_power)
  node = FuzzyAssignExpr(array=X, centers=C)
  node.exponent, node.eps, node.weight_power = exponent, eps, weight_power
  parts = []
  for part in (0, 1, 2):
    e = FuzzyPartExpr(step=node)
    e.part, e.nkd = part, (X.shape[0], C.shape[0], X.shape[1])
    parts.append(e)
  return tuple(parts)


def fuzzy_membership(X, C, m=2.0, eps=1e-11):
  """The (n, k) membership matrix U of ``fuzzy_assign``'s rule, lazily, in X's
  dtype, tiled in row slabs at X's row cuts.  Every row sums to 1."""
  X, C, exponent, eps, _ = _checked('fuzzy_membership', X, C, m, eps, 1.0)
  node = FuzzyMembershipExpr(array=X, centers=C)
  node.exponent, node.eps, node.weight_power = exponent, eps, 1.0
  return node


# ------------------------------------------------------------- evaluation
def _points(t):
  return t if t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1) else backend.get().contiguous(t)


def fuzzy_step_arrays(arr, centers, exponent, eps, weight_power, want_U):
  """The arrays (labels, counts, sums) -- with ``want_U`` the array U alone --
  of the dense array ``arr`` against ``centers``.  Collective."""
  ctx = runtime.get()
  be = backend.get()
  arr = with_tiles(arr)
  c = be.contiguous(whole(with_tiles(centers)), np.float64)
  n, d = arr.shape
  k = int(c.shape[0])
  if arr.replicated:  # held in full by every rank: so are the results
    lab, U, sums, counts = be.fuzzy_step(_points(arr.device_data()), c, exponent, eps, weight_power, not want_U, want_U)
    if want_U:
      return distarray.ReplicatedArray(U)
    return tuple(distarray.ReplicatedArray(t) for t in (lab, counts, sums))
  sl, got = gather_slabs(arr, 0)  # row slabs at arr's row cuts, each on the owner of its first tile
  sums = counts = None
  rows = {}
  for qi in sorted(got):
    lab, U, sums, counts = be.fuzzy_step(_points(got[qi]), c, exponent, eps, weight_power, not want_U, want_U,
                                         sums=sums, counts=counts)  # the first writes the buffers, the others add
    rows[qi] = U if want_U else lab
  tail = (k,) if want_U else ()
  tiles = {ext.create((e.ul[0],) + (0,) * len(tail), (e.lr[0],) + tail, (n,) + tail): w for e, w in sl}
  local = {ext.create((e.ul[0],) + (0,) * len(tail), (e.lr[0],) + tail, (n,) + tail): rows[qi]
           for qi, (e, w) in enumerate(sl) if qi in rows}
  out = distarray.from_tiles((n,) + tail, arr.dtype if want_U else np.int64, tiles, local)
  if want_U:
    return out
  if sums is None:  # no row slab on this rank
    import torch
    sums = torch.zeros((k, d), dtype=torch.float64, device=ctx.device)
    counts = torch.zeros((k,), dtype=torch.float64, device=ctx.device)
  comm.all_reduce(counts, 'sum')
  comm.all_reduce(sums, 'sum')
  w0 = sl[0][1]
  tc = deferred((k,), np.float64, {ext.from_shape((k,)): w0})
  ts = deferred((k, d), np.float64, {ext.from_shape((k, d)): w0})
  combine.deliver(tc, counts)
  combine.deliver(ts, sums)
  return out, tc, ts

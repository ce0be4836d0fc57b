"""``nbody_accel``: gravitational accelerations by direct summation on
spx_nbody_accel.

The reference's driver (spartan/examples/nbody.py ``move``) writes one time step
as about a dozen (n, n) arrays: the three coordinate differences, the distance,
the clamp mask, three force components, their ``set_diagonal`` copies and three
``sum(axis=0)`` passes.  None of them is built here.  For every body j

    a_j = sum_i G m_i (p_i - p_j) / r_ij^3,   r_ij = max(|p_i - p_j|, rmin),

out of one kernel that reads 4 n values and writes 3 n.  The term of i = j (and
of two bodies at one position) is exactly 0 for rmin > 0: d = 0 and r = rmin.

``nbody_accel(x, y, z, m)`` is a lazy triple ``(ax, ay, az)`` hanging off one
node: forcing any of them runs the summation once.

Routes; every rank issues the same exchanges whether or not it owns bodies:

  * x, y, z and m are gathered in full to every rank (``blocks.whole``, the
    route of the fuzzy step's centres): they are the sources;
  * replicated operands are computed whole on every rank; the results are
    replicated;
  * otherwise the targets are cut at x's row cuts; the targets of a slab are
    slices of the gathered arrays, so y, z and m may be tiled in any way.  The
    owner of a slab's first tile issues one launch for it; ``ax, ay, az`` are
    tiled at x's row cuts on those owners.

Not built: targets other than the bodies themselves, a source set too large to
replicate on one GPU, any sub-quadratic method.
"""
import numpy as np

from .. import backend, runtime
from ..array import distarray
from ..array import extent as ext
from ..array.blocks import slabs, whole, with_tiles
from .base import Expr, as_array

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
G_DEFAULT = 6.67384e-11


class NbodyTriple:
  """The value of an ``NbodyAccelExpr``: the arrays ax, ay, az (shape and
  dtype: theirs)."""

  def __init__(self, ax, ay, az):
    self.parts = (ax, ay, az)
    self.shape, self.dtype = tuple(ax.shape), np.dtype(ax.dtype)


class NbodyAccelExpr(Expr):
  _members = ('x', 'y', 'z', 'm')

  def compute_shape(self):
    return tuple(self.x.shape)

  def compute_dtype(self):
    return np.dtype(self.x.dtype)

  def pretty_str(self):
    return 'NbodyAccel[%d](%s, %s, %s, %s, G=%r, rmin=%r)' % (self.expr_id, self.x, self.y, self.z, self.m, self.G,
                                                                self.rmin)

  def _evaluate(self, deps):
    return NbodyTriple(*nbody_arrays(*(distarray.as_array(deps[k]) for k in self._members), self.G, self.rmin))


class NbodyPartExpr(Expr):
  """ax (``part`` 0), ay (1) or az (2) of an ``NbodyAccelExpr``."""
  _members = ('step',)

  def compute_shape(self):
    return tuple(self.step.shape)

  def compute_dtype(self):
    return np.dtype(self.step.dtype)

  def pretty_str(self):
    return '%s(%s)' % (('ax', 'ay', 'az')[self.part], self.step)

  def _evaluate(self, deps):
    return deps['step'].parts[self.part]


def nbody_accel(x, y, z, m, G=G_DEFAULT, rmin=1.0):
  """``(ax, ay, az)``, lazily: the accelerations of n bodies at the (n,)
  float32 / float64 positions ``x, y, z`` with masses ``m`` under each other's
  gravity, ``a_j = sum_i G m_i (p_i - p_j) / r_ij^3`` with every distance below
  ``rmin`` taken as ``rmin`` (so a body exerts nothing on itself, nor on a body
  at its own position; ``rmin = 0`` makes those terms 0 / 0).  Each output is
  (n,) in the inputs' dtype, tiled at x's row cuts.  The three share one
  evaluation; no (n, n) array is built.  A NaN position or mass makes every
  output NaN."""
  from .sparse import is_sparse
  if any(is_sparse(a) for a in (x, y, z, m)):
    raise TypeError('nbody_accel: a sparse array is not accepted here: convert it with todense() first')
  x, y, z, m = (as_array(a) for a in (x, y, z, m))
  for name, a in zip('xyzm', (x, y, z, m)):
    if len(a.shape) != 1:
      raise ValueError('nbody_accel: %s must be 1-d, got shape %s' % (name, tuple(a.shape)))
    if a.shape[0] != x.shape[0]:
      raise ValueError('nbody_accel: x, y, z and m must have one length, got %d for x and %d for %s'
                       % (x.shape[0], a.shape[0], name))
  dt = np.dtype(x.dtype)
  for name, a in zip('xyzm', (x, y, z, m)):
    if np.dtype(a.dtype) not in _FLOATS:
      raise ValueError('nbody_accel: %s has dtype %s; float32 / float64 are served: convert it with astype'
                       % (name, np.dtype(a.dtype)))
    if np.dtype(a.dtype) != dt:
      raise ValueError('nbody_accel: x, y, z and m must have one dtype, got %s for x and %s for %s: convert with '
                       'astype' % (dt, np.dtype(a.dtype), name))
  G, rmin = float(G), float(rmin)
  if not np.isfinite(G):
    raise ValueError('nbody_accel: G = %r is not finite' % G)
  if not (rmin >= 0.0 and np.isfinite(rmin)):
    raise ValueError('nbody_accel: rmin = %r is not finite and >= 0' % rmin)
  node = NbodyAccelExpr(x=x, y=y, z=z, m=m)
  node.G, node.rmin = G, rmin
  parts = []
  for part in (0, 1, 2):
    e = NbodyPartExpr(step=node)
    e.part = part
    parts.append(e)
  return tuple(parts)


# ------------------------------------------------------------- evaluation
def nbody_arrays(x, y, z, m, G, rmin):
  """The arrays (ax, ay, az) of the dense 1-d arrays x, y, z, m.  Collective."""
  ctx = runtime.get()
  be = backend.get()
  x, y, z, m = (with_tiles(a) for a in (x, y, z, m))
  sx, sy, sz, sm = (whole(a) for a in (x, y, z, m))  # the sources: every body on every rank
  n = int(x.shape[0])
  if x.replicated:  # held in full by every rank: so are the results
    return tuple(distarray.ReplicatedArray(t) for t in be.nbody_accel(sx, sy, sz, sx, sy, sz, sm, G, rmin))
  sl = slabs(x, 0)  # the target slabs at x's row cuts, each on the owner of its first tile
  tiles = {ext.create((e.ul[0],), (e.lr[0],), (n,)): w for e, w in sl}
  local = ({}, {}, {})
  for e, w in sl:
    if not ctx.is_local(w):
      continue
    lo, hi = e.ul[0], e.lr[0]
    got = be.nbody_accel(sx[lo:hi], sy[lo:hi], sz[lo:hi], sx, sy, sz, sm, G, rmin)
    for part, t in zip(local, got):
      part[ext.create((lo,), (hi,), (n,))] = t
  return tuple(distarray.from_tiles((n,), x.dtype, tiles, part) for part in local)

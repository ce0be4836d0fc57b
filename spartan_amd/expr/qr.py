"""``qr``: NumPy's reduced QR of a tall or square matrix on spx_geqr /
spx_orgqr.

The reference's ``spartan/examples/ssvd/qr.py`` forms Y'Y, takes a host
Cholesky factor and its inverse, and multiplies once more (CholeskyQR): it
loses orthogonality as cond(Y)^2 u.  The contract here is NumPy's
``qr(mode='reduced')`` -- Q (m, n) with orthonormal columns, R (n, n) upper
triangular, A = Q R -- by Householder reflectors, backward stable for any
conditioning and any rank, with diag(R) >= 0 (which makes the pair unique for a
full-rank A and the same on every route up to rounding).

Routes; every rank issues the same exchanges whether or not it owns tiles:

  * a replicated array, or an array in one tile, is factored on its holder;
  * every tile spans axis 1 (row slabs): the distributed TSQR.  Each rank
    runs ``geqr`` on each of its tiles; the per-tile Rs are gathered to every
    rank (ONE exchange of T n x n numbers in total, in tile order); every rank
    factors that stack identically, so R is already replicated; every rank
    forms the stack's Q with the sign matrix D as its seed and seeds ``orgqr``
    of each of its own tiles with that tile's n x n slice.  Q keeps A's
    tiling; no tile of A or Q ever leaves its owner.  (A tile with fewer than
    n rows is not factored: its rows go on the stack as they are and its rows
    of Q are its rows of the stack's Q);
  * any other layout (tiles cut along axis 1): the row slabs of
    ``blocks.gather_slabs(arr, 0)`` (``array/blocks.py``, route 3) go through
    the route above and are delivered into A's tiling by one
    ``scatter_slabs``.

Both results hang off one ``QRExpr`` node: forcing either evaluates the
factorization once.
"""
import numpy as np

from .. import backend, runtime
from ..array import distarray
from ..array import extent as ext
from ..array.blocks import deferred, gather_slabs, scatter_slabs, spans, whole, with_tiles
from .base import Expr, as_array

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


class QRPair:
  """The value of a ``QRExpr``: the arrays Q and R (shape and dtype: Q's)."""

  def __init__(self, Q, R):
    self.Q, self.R = Q, R
    self.shape, self.dtype = tuple(Q.shape), np.dtype(Q.dtype)


class QRExpr(Expr):
  _members = ('array',)

  def compute_shape(self):
    return self.array.shape

  def compute_dtype(self):
    return np.dtype(self.array.dtype)

  def pretty_str(self):
    return 'QR[%d](%s)' % (self.expr_id, self.array)

  def _evaluate(self, deps):
    return QRPair(*qr_array(distarray.as_array(deps['array'])))


class QRPartExpr(Expr):
  """Q (``part`` 0) or R (``part`` 1) of a ``QRExpr``."""
  _members = ('pair',)

  def compute_shape(self):
    m, n = self.pair.shape
    return (m, n) if self.part == 0 else (n, n)

  def compute_dtype(self):
    return np.dtype(self.pair.dtype)

  def pretty_str(self):
    return '%s(%s)' % ('QR'[self.part], self.pair)

  def _evaluate(self, deps):
    p = deps['pair']
    return p.Q if self.part == 0 else p.R


def qr(A):
  """``(Q, R)``, lazily: the reduced QR factorization of the (m, n) float32 /
  float64 matrix ``A``, m >= n (NumPy's ``mode='reduced'``).  Q is (m, n) in
  A's dtype and tiling, R is (n, n), upper triangular with diag(R) >= 0,
  replicated."""
  A = as_array(A)
  if len(A.shape) != 2:
    raise ValueError('qr: a 2-d array is needed, got shape %s' % (tuple(A.shape),))
  dt = np.dtype(A.dtype)
  if dt not in _FLOATS:
    raise TypeError('qr: dtype %s is not float32 / float64' % dt)
  m, n = A.shape
  if m < n:
    raise NotImplementedError('qr: a tall or square matrix is needed (m >= n), got shape %s' % ((m, n),))
  nmax, _ = backend.geqr_plan(dt, n)
  if n > nmax:
    raise NotImplementedError('qr: %d columns are above the limit of %d for %s' % (n, nmax, dt))
  node = QRExpr(array=A)
  parts = []
  for part in (0, 1):
    e = QRPartExpr(pair=node)
    e.part = part
    parts.append(e)
  return tuple(parts)


# ------------------------------------------------------------- evaluation
def _nonneg(R):
  """(D R, D) for D = diag(sign(diag R)) (+1 for a zero), as device tensors."""
  import torch
  d = torch.where(torch.diagonal(R) < 0, -torch.ones_like(R[0]), torch.ones_like(R[0]))
  return R * d[:, None], torch.diag(d)


def _qr_block(t):
  """(Q, R) of the device block ``t`` (m >= n), diag(R) >= 0."""
  import torch
  be = backend.get()
  src = be.contiguous(t)
  R, h = be.geqr(src)
  R, D = _nonneg(R)
  Q = torch.empty_like(src)
  be.orgqr(h, D, Q)
  return Q, R


def _tsqr(dtype, n, pieces):
  """The distributed TSQR over row slabs.  ``pieces``: [(rows, worker, device
  block or None)] in row order, the block given where the worker is local.
  A slab of at least n rows puts its n x n R on the stack; a shorter one puts
  its own rows there (its Q is the identity: padding it with zero rows instead
  would cut rows off an orthogonal factor, which only a full-rank R forgives).
  Returns ({piece index: that piece's rows of Q} for the local pieces, R).
  Collective: one gather of the stack."""
  import torch
  ctx = runtime.get()
  be = backend.get()
  offs = [0]
  for rows, _w, _b in pieces:
    offs.append(offs[-1] + min(rows, n))
  stack_shape = (offs[-1], n)
  tiles, local, handles = {}, {}, {}
  for t, (rows, w, block) in enumerate(pieces):
    e = ext.create((offs[t], 0), (offs[t + 1], n), stack_shape)
    tiles[e] = w
    if not ctx.is_local(w):
      continue
    src = be.contiguous(block)
    if rows < n:
      local[e] = src
    else:
      local[e], handles[t] = be.geqr(src)
  S = whole(distarray.from_tiles(stack_shape, dtype, tiles, local))
  R, top = be.geqr(S)  # the same bits on every rank
  R, D = _nonneg(R)
  seeds = torch.empty(stack_shape, dtype=S.dtype, device=S.device)
  be.orgqr(top, D, seeds)
  out = {}
  for t, (rows, w, _b) in enumerate(pieces):
    if not ctx.is_local(w):
      continue
    seed = seeds[offs[t]:offs[t + 1]]
    if rows < n:
      out[t] = seed.clone()
    else:
      out[t] = torch.empty((rows, n), dtype=S.dtype, device=S.device)
      be.orgqr(handles[t], seed, out[t])
  return out, R


def qr_array(arr):
  """(Q, R) arrays of the array ``arr``."""
  ctx = runtime.get()
  arr = with_tiles(arr)
  m, n = arr.shape
  dt = np.dtype(arr.dtype)
  if arr.replicated:  # held in full by every rank
    Q, R = _qr_block(arr.device_data())
    return distarray.ReplicatedArray(Q), distarray.ReplicatedArray(R)
  if len(arr.tiles) == 1:
    (e, w), = arr.tiles.items()
    src = ctx.owner(w)
    local = {}
    R = None
    if src == ctx.rank:
      local[e], R = _qr_block(arr.fetch(e))
    Q = distarray.from_tiles(arr.shape, dt, arr.tiles, local)
    # R to every rank: a one-tile array gathered in full
    rt = {ext.from_shape((n, n)): w}
    rarr = distarray.from_tiles((n, n), dt, rt, {k: R for k in rt} if R is not None else {})
    return Q, distarray.ReplicatedArray(whole(rarr))
  if spans(arr, (1,)):
    order = sorted(arr.tiles, key=lambda e: e.ul[0])
    pieces = [(e.shape[0], arr.tiles[e], arr.fetch(e) if ctx.is_local(arr.tiles[e]) else None) for e in order]
    qs, R = _tsqr(dt, n, pieces)
    Q = distarray.from_tiles(arr.shape, dt, arr.tiles, {order[t]: q for t, q in qs.items()})
    return Q, distarray.ReplicatedArray(R)
  slabs, got = gather_slabs(arr, 0)
  pieces = [(e.shape[0], w, got.get(qi)) for qi, (e, w) in enumerate(slabs)]
  qs, R = _tsqr(dt, n, pieces)
  target = deferred(arr.shape, dt, arr.tiles)
  scatter_slabs(target, slabs, qs)
  return target, distarray.ReplicatedArray(R)

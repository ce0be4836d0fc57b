"""``eigh`` / ``eigvalsh``: NumPy's symmetric eigen-decomposition on spx_syevj
(DESIGN.md 3.21).

``eigh(A, UPLO)`` is ``np.linalg.eigh``: for a symmetric (n, n) matrix, or a
stack (B, n, n) of them, the eigenvalues w in ascending order and the
eigenvectors as the columns of V, A V = V diag(w), from the triangle ``UPLO``
names.  n is at most ``backend.syevj_plan(dtype)[0]`` (128 for float32, 96 for
float64): one workgroup holds a matrix and its vectors in LDS and runs a
parallel cyclic Jacobi method on them; a batch is a grid of such workgroups.
Every column of V has its entry of largest magnitude positive, so the pair is
the same bits on every route.

Routes; every rank issues the same exchanges whether or not it owns tiles:

  * 2-d, replicated: computed on its holder; w and V are replicated;
  * 2-d, tiled in any way: ONE ``gather_regions`` of the whole matrix (at most
    128 KiB) to every rank, every rank runs the same kernel on the same bits;
    w and V are replicated, with the same bits on every rank and for every
    tile layout;
  * 3-d, every tile spans axes 1 and 2 (batch slabs): each rank runs one
    ``syevj`` per tile it owns; V keeps A's tiling, w (B, n) is cut along axis
    0 at the same places on the same workers; nothing leaves its owner;
  * 3-d, any other layout: the batch slabs of ``blocks.gather_slabs(arr, 0)``
    (``array/blocks.py``, route 3) are computed on their owners, and V is
    delivered into A's tiling by one ``scatter_slabs``; w is tiled by the
    slabs;
  * 3-d, replicated: computed on the holder.

``info`` of every ``syevj`` stays on the device until the end of the
evaluation: the smallest entry over all matrices and ranks is then read once,
and a -1 (a matrix that did not converge, or one that is not finite) raises
``np.linalg.LinAlgError('Eigenvalues did not converge')`` on every rank.

Both results hang off one ``EighExpr`` node: forcing either runs the kernel
once.
"""
import numpy as np

from .. import backend, comm, runtime
from ..array import distarray
from ..array import extent as ext
from ..array.blocks import deferred, gather_slabs, scatter_slabs, spans, whole, with_tiles
from .base import Expr, as_array

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


class EighPair:
  """The value of an ``EighExpr``: the arrays w and V (shape and dtype: V's)."""

  def __init__(self, w, V):
    self.w, self.V = w, V
    self.shape, self.dtype = tuple(V.shape), np.dtype(V.dtype)


class EighExpr(Expr):
  _members = ('array',)

  def compute_shape(self):
    return self.array.shape

  def compute_dtype(self):
    return np.dtype(self.array.dtype)

  def pretty_str(self):
    return 'Eigh[%d](%s, UPLO=%s)' % (self.expr_id, self.array, self.uplo)

  def _evaluate(self, deps):
    return EighPair(*eigh_array(distarray.as_array(deps['array']), self.uplo))


class EighPartExpr(Expr):
  """w (``part`` 0) or V (``part`` 1) of an ``EighExpr``."""
  _members = ('pair',)

  def compute_shape(self):
    s = tuple(self.pair.shape)
    return s[:-1] if self.part == 0 else s

  def compute_dtype(self):
    return np.dtype(self.pair.dtype)

  def pretty_str(self):
    return '%s(%s)' % ('wV'[self.part], self.pair)

  def _evaluate(self, deps):
    p = deps['pair']
    return p.w if self.part == 0 else p.V


def eigh(A, UPLO='L'):
  """``(w, V)``, lazily: the eigenvalues (ascending) and eigenvectors (the
  columns of V) of the symmetric float32 / float64 matrix ``A`` of shape (n, n),
  or of every matrix of a stack (B, n, n); only the triangle ``UPLO`` ('L' or
  'U') is read.  Evaluation raises ``np.linalg.LinAlgError`` for a matrix that
  holds a non-finite value or does not converge."""
  if UPLO not in ('L', 'U'):
    raise ValueError("eigh: UPLO must be 'L' or 'U', not %r" % (UPLO,))
  A = as_array(A)
  shape = tuple(A.shape)
  if len(shape) not in (2, 3) or shape[-1] != shape[-2]:
    raise ValueError('eigh: a square matrix (n, n) or a stack (B, n, n) is needed, got shape %s' % (shape,))
  dt = np.dtype(A.dtype)
  if dt not in _FLOATS:
    raise TypeError('eigh: dtype %s is not float32 / float64' % dt)
  nmax, _ = backend.syevj_plan(dt)
  if shape[-1] > nmax:
    raise NotImplementedError('eigh: n = %d is above the limit of %d for %s' % (shape[-1], nmax, dt))
  node = EighExpr(array=A)
  node.uplo = UPLO
  parts = []
  for part in (0, 1):
    e = EighPartExpr(pair=node)
    e.part = part
    parts.append(e)
  return tuple(parts)


def eigvalsh(A, UPLO='L'):
  """The eigenvalues of ``eigh(A, UPLO)``, lazily."""
  return eigh(A, UPLO)[0]


# ------------------------------------------------------------- evaluation
def _raise_on_info(infos):
  """``infos``: the info tensors of this rank's syevj calls.  The smallest
  entry over all ranks is read (the evaluation's one host read); a negative
  one raises.  Collective."""
  import torch
  ctx = runtime.get()
  worst = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
  for info in infos:
    if info.numel():
      worst = torch.minimum(worst, info.to(torch.int64).min().reshape(1))
  worst = comm.all_reduce(worst, 'min')
  if int(worst.item()) < 0:
    raise np.linalg.LinAlgError('Eigenvalues did not converge')


def _block(t, uplo, infos):
  """(w, V) of the device block ``t``; its info joins ``infos``."""
  be = backend.get()
  w, V, info = be.syevj(be.contiguous(t), uplo)
  infos.append(info)
  return w, V


def eigh_array(arr, uplo='L'):
  """(w, V) arrays of the array ``arr``."""
  ctx = runtime.get()
  arr = with_tiles(arr)
  dt = np.dtype(arr.dtype)
  n = arr.shape[-1]
  infos = []
  if arr.replicated:  # held in full by every rank
    w, V = _block(arr.device_data(), uplo, infos)
    _raise_on_info(infos)
    return distarray.ReplicatedArray(w), distarray.ReplicatedArray(V)
  if arr.ndim == 2:
    w, V = _block(whole(arr), uplo, infos)  # the same bits on every rank
    _raise_on_info(infos)
    return distarray.ReplicatedArray(w), distarray.ReplicatedArray(V)
  nb = arr.shape[0]
  wshape = (nb, n)

  def wext(e):
    return ext.create((e.ul[0], 0), (e.lr[0], n), wshape)

  if spans(arr, (1, 2)):
    wl, vl = {}, {}
    for e, wk in arr.tiles.items():
      if ctx.is_local(wk):
        wl[wext(e)], vl[e] = _block(arr.fetch(e), uplo, infos)
    _raise_on_info(infos)
    return (distarray.from_tiles(wshape, dt, {wext(e): wk for e, wk in arr.tiles.items()}, wl),
            distarray.from_tiles(arr.shape, dt, arr.tiles, vl))
  slabs, got = gather_slabs(arr, 0)
  target = deferred(arr.shape, dt, arr.tiles)
  wl, vs = {}, {}
  for qi, t in got.items():
    wl[wext(slabs[qi][0])], vs[qi] = _block(t, uplo, infos)
  scatter_slabs(target, slabs, vs)
  _raise_on_info(infos)
  return distarray.from_tiles(wshape, dt, {wext(e): wk for e, wk in slabs}, wl), target

"""``cholesky`` / ``solve_triangular`` / ``cho_solve``: dense linear algebra on
spx_potrf / spx_trsm / spx_syrk.

The reference's ``spartan/examples/cholesky.py`` runs a tiled right-looking
factorization whose three mappers call scipy's LAPACK / BLAS per tile.  Its
result -- the lower factor with zeros above the diagonal -- is the contract
here, for ANY tile layout:

  * a replicated array, or an array in one tile, is factored on its holder;
  * a p x p tile grid whose row cuts equal its column cuts (the reference's
    precondition) runs the reference's loop with every tile operation on the
    tile's owner: for k = 0 .. p-1, ``potrf`` on tile (k, k); L_kk gathered
    to the owners of the tiles below it, which solve X L_kk^T = A_ik there
    (``trsm`` RIGHT/T); the solved panel tiles gathered to the owners of the
    trailing tiles, which subtract P_i P_j^T (``syrk``, ``lower`` on the
    diagonal tiles).  Two ``gather_regions`` exchanges a step; tiles above the
    diagonal are zero-filled; the result keeps the input's tiling;
  * any other layout is gathered to one owner (it must fit that GPU), factored
    there and delivered into the input's tiling by one ``scatter_slabs``
    (``array/blocks.py``).

``info`` of every ``potrf`` stays on the device until the end of the
evaluation: the first failed order over all tiles and ranks is then read once
and raised as ``np.linalg.LinAlgError``.

``solve_triangular(L, B, trans)`` solves op(L) X = B for the lower-triangular
L.  The right-hand-side columns are independent and each needs all of L: L is
gathered in full to every rank that owns a slab of B (``blocks.whole``), and B
takes the three routes of ``array/blocks.py`` with axis 0 (a tile spanning axis
0 is solved on its owner; otherwise B is cut into column slabs).

Every rank issues the same exchanges whether or not it owns tiles.
"""
import numpy as np

from .. import backend, comm, runtime
from ..array import distarray
from ..array import extent as ext
from ..array.blocks import deferred, gather_slabs, map_blocks, scatter_slabs, slabs, whole, with_tiles
from .base import Expr, as_array

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
_NO_INFO = np.iinfo(np.int64).max


class CholeskyExpr(Expr):
  _members = ('array',)

  def compute_shape(self):
    return self.array.shape

  def compute_dtype(self):
    return np.dtype(self.array.dtype)

  def pretty_str(self):
    return 'Cholesky[%d](%s)' % (self.expr_id, self.array)

  def _evaluate(self, deps):
    return cholesky_array(distarray.as_array(deps['array']))


class SolveTriangularExpr(Expr):
  _members = ('L', 'B')

  def compute_shape(self):
    return self.B.shape

  def compute_dtype(self):
    return np.dtype(self.B.dtype)

  def pretty_str(self):
    return 'SolveTriangular[%d](%s, %s, trans=%d)' % (self.expr_id, self.L, self.B, self.trans)

  def _evaluate(self, deps):
    return solve_triangular_array(distarray.as_array(deps['L']), distarray.as_array(deps['B']), self.trans)


def _check_square(a, name):
  if len(a.shape) != 2 or a.shape[0] != a.shape[1]:
    raise ValueError('%s: a square 2-d array is needed, got shape %s' % (name, tuple(a.shape)))
  if np.dtype(a.dtype) not in _FLOATS:
    raise TypeError('%s: dtype %s is not float32 / float64' % (name, np.dtype(a.dtype)))


def cholesky(A):
  """The lower Cholesky factor L of the symmetric positive definite ``A``
  (A = L L^T; only A's lower triangle is read, L is zero above the diagonal),
  lazily.  Evaluation raises ``np.linalg.LinAlgError`` naming the order of the
  first leading minor that is not positive definite."""
  A = as_array(A)
  _check_square(A, 'cholesky')
  return CholeskyExpr(array=A)


def solve_triangular(L, B, trans=0, lower=True):
  """X with op(L) X = B for the lower-triangular ``L``: ``trans`` 0 / 'N'
  solves L X = B, 1 / 'T' solves L^T X = B.  ``B`` is (n,) or (n, m); the
  result has B's shape and dtype.  No singularity check (a zero diagonal gives
  inf / NaN)."""
  if trans not in (0, 1, 'N', 'T'):
    raise ValueError("solve_triangular: trans %r is not one of 0, 1, 'N', 'T'" % (trans,))
  trans = 1 if trans in (1, 'T') else 0
  if not lower:
    raise NotImplementedError(
        'solve_triangular: upper-triangular storage is not supported; for U = L^T pass L with trans=%d'
        % (1 - trans))
  L = as_array(L)
  B = as_array(B)
  _check_square(L, 'solve_triangular')
  if len(B.shape) not in (1, 2) or B.shape[0] != L.shape[0]:
    raise ValueError('solve_triangular: B of shape %s against L of shape %s' % (tuple(B.shape), tuple(L.shape)))
  if np.dtype(B.dtype) != np.dtype(L.dtype):
    raise TypeError('solve_triangular: L is %s and B is %s; mixed dtypes are not supported'
                    % (np.dtype(L.dtype), np.dtype(B.dtype)))
  e = SolveTriangularExpr(L=L, B=B)
  e.trans = trans
  return e


def cho_solve(L, B):
  """X with (L L^T) X = B, from the Cholesky factor ``L``: two solves."""
  return solve_triangular(L, solve_triangular(L, B, trans=0), trans=1)


# ------------------------------------------------------------- evaluation
def _raise_on_info(infos):
  """``infos``: [(row offset, info tensor)] of this rank's potrf calls.  The
  first failed order over all ranks is read (the evaluation's one host read)
  and raised.  Collective."""
  import torch
  ctx = runtime.get()
  first = torch.full((1,), _NO_INFO, dtype=torch.int64, device=ctx.device)
  for off, info in infos:
    order = info.to(torch.int64) + int(off)
    first = torch.minimum(first, torch.where(info > 0, order, torch.full_like(order, _NO_INFO)))
  first = comm.all_reduce(first, 'min')
  order = int(first.item())
  if order != _NO_INFO:
    raise np.linalg.LinAlgError('cholesky: the leading minor of order %d is not positive definite' % order)


def _potrf_block(t):
  """(L, info) of the square device block ``t`` (left untouched)."""
  import torch
  be = backend.get()
  src = be.contiguous(t)
  L = torch.empty_like(src)
  return L, be.potrf(src, L)


def _square_grid(arr):
  """The cuts of a p x p (p > 1) tile grid whose row cuts equal its column
  cuts, else None."""
  rows = sorted({(e.ul[0], e.lr[0]) for e in arr.tiles})
  cols = sorted({(e.ul[1], e.lr[1]) for e in arr.tiles})
  p = len(rows)
  if p < 2 or rows != cols or len(arr.tiles) != p * p:
    return None
  have = {(e.ul[0], e.lr[0], e.ul[1], e.lr[1]) for e in arr.tiles}
  if have != {(r[0], r[1], c[0], c[1]) for r in rows for c in cols}:
    return None
  return rows


def _cholesky_tiled(arr, cuts):
  import torch
  ctx = runtime.get()
  be = backend.get()
  p = len(cuts)
  n = arr.shape[0]
  ex = {(i, j): ext.create((cuts[i][0], cuts[j][0]), (cuts[i][1], cuts[j][1]), (n, n))
        for i in range(p) for j in range(p)}
  own = {ij: ctx.owner(arr.tiles[e]) for ij, e in ex.items()}
  me = ctx.rank
  tdt = backend.torch_dtype(arr.dtype)
  data = {}
  for (i, j), e in ex.items():
    if own[i, j] != me:
      continue
    if j > i:
      data[e] = torch.zeros(e.shape, dtype=tdt, device=ctx.device)
    else:
      data[e] = be.contiguous(arr.fetch(e)).clone()  # the work copy: updated in place
  work = distarray.from_tiles(arr.shape, arr.dtype, arr.tiles, data)
  infos = []
  for k in range(p):
    ekk = ex[k, k]
    if own[k, k] == me:
      t = data[ekk]
      infos.append((cuts[k][0], be.potrf(t, t)))
    if k == p - 1:
      break
    # L_kk to the owners of the column's tiles
    dsts = sorted({own[i, k] for i in range(k + 1, p)})
    got = distarray.gather_regions(work, [(ekk, d) for d in dsts])
    if me in dsts:
      lkk = be.contiguous(got[dsts.index(me)])
      for i in range(k + 1, p):
        if own[i, k] == me:
          be.trsm(lkk, data[ex[i, k]], side='R', trans=True)
    # panel tile i to the owners of the trailing tiles of row i and of column i
    reqs = []
    for i in range(k + 1, p):
      need = {own[i, j] for j in range(k + 1, i + 1)} | {own[r, i] for r in range(i, p)}
      reqs.extend((i, d) for d in sorted(need))
    got = distarray.gather_regions(work, [(ex[i, k], d) for i, d in reqs])
    panel = {i: be.contiguous(got[q]) for q, (i, d) in enumerate(reqs) if d == me}
    for i in range(k + 1, p):
      for j in range(k + 1, i + 1):
        if own[i, j] == me:
          be.syrk(panel[i], panel[j], data[ex[i, j]], lower=(i == j))
  _raise_on_info(infos)
  return work


def cholesky_array(arr):
  ctx = runtime.get()
  arr = with_tiles(arr)
  _check_square(arr, 'cholesky')
  if arr.replicated:  # held in full by every rank
    L, info = _potrf_block(arr.device_data())
    _raise_on_info([(0, info)])
    return distarray.ReplicatedArray(L)
  if len(arr.tiles) == 1:
    (e, w), = arr.tiles.items()
    local, infos = {}, []
    if ctx.is_local(w):
      local[e], info = _potrf_block(arr.fetch(e))
      infos.append((0, info))
    _raise_on_info(infos)
    return distarray.from_tiles(arr.shape, arr.dtype, arr.tiles, local)
  cuts = _square_grid(arr)
  if cuts is not None:
    return _cholesky_tiled(arr, cuts)
  sl, got = gather_slabs(arr, None)  # the whole matrix on the owner of its first tile
  target = deferred(arr.shape, arr.dtype, arr.tiles)
  Ls, infos = {}, []
  for qi, t in got.items():
    Ls[qi], info = _potrf_block(t)
    infos.append((0, info))
  scatter_slabs(target, sl, Ls)
  _raise_on_info(infos)
  return target


def _solve_block(lfull, t, shape, trans):
  """op(L) X = the device block ``t`` of ``shape`` ((n,) or (n, w)); a copy."""
  be = backend.get()
  n = shape[0]
  w = shape[1] if len(shape) == 2 else 1
  x = be.contiguous(t).clone().reshape(n, w)
  be.trsm(lfull, x, side='L', trans=bool(trans))
  return x.reshape(tuple(shape))


def solve_triangular_array(L, B, trans):
  ctx = runtime.get()
  L = with_tiles(L)
  B = with_tiles(B)
  p = 1 if B.ndim == 2 else None
  # L to every rank that solves, before B moves: all ranks for a replicated B, else the owners of B's column
  # slabs (the tiles themselves where every tile spans axis 0)
  lfull = whole(L, None if B.replicated else {ctx.owner(w) for _e, w in slabs(B, p)})
  return map_blocks(B, (0,), p, lambda t, shape: _solve_block(lfull, t, shape, trans))

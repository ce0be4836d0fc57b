"""``svd`` / ``svdvals`` / ``pinv``: NumPy's reduced singular value
decomposition on spx_gesvj.

``svd(A)`` is ``np.linalg.svd(A, full_matrices=False)``: for an (m, n) matrix,
or a stack (B, m, n), with k = min(m, n), U (.., m, k), s (.., k) descending and
non-negative, Vt (.., k, n), A = U diag(s) Vt.  One workgroup holds a matrix
and its right vectors in LDS and runs a one-sided Jacobi method on its columns;
it never forms a Gram matrix, so small singular values keep their relative
accuracy.

Two rules make the triple unique:

  * the sign rule is stated on the square k x k factor (Vt when m >= n, U when
    m < n): the entry of largest magnitude (the first on a tie) of each of its
    singular vectors is positive, and the other factor follows.  So, for
    m != n, ``svd(transpose(A))`` is ``(Vt^T, s, U^T)`` of ``svd(A)``, and no
    route needs a column argmax over a distributed factor;
  * for an exactly zero singular value the vector in the LONG factor (U when
    m >= n) is exactly zero -- LAPACK gesvj's contract, a deviation from NumPy.
    A = U diag(s) Vt holds regardless, and the square factor is orthogonal.

Routes; every rank issues the same exchanges whether or not it owns tiles:

  * wide (m < n): the transposed problem (a zero-copy view) goes through the
    routes below and the roles of U and Vt are swapped;
  * 2-d direct (the long side is at most ``gesvj_plan(dtype, short)[1]``): ONE
    ``whole()`` of the matrix to every rank (none for a replicated array),
    every rank runs the same kernel; U, s and Vt are replicated, with the same
    bits on every rank and for every tile layout;
  * 2-d tall (m above that limit; n within ``geqr_plan``'s): ``qr_array`` gives
    Q in A's tiling and the replicated R, every rank runs ``gesvj(R)``
    identically, s and Vt are replicated and U = Q U_R is formed on the owners
    of Q's tiles by the GEMM (tile by tile where every tile of Q holds whole
    rows, ``run_dot`` otherwise).  The TSQR tree depends on the layout, so this
    route gives the same triple up to rounding only;
  * 3-d stack (the long side within the direct limit): batch slabs stay on
    their owners when every tile spans axes 1 and 2, any other layout goes
    through ``gather_slabs(arr, 0)``; U, s and Vt are tiled along axis 0 at the
    slab cuts on the slabs' workers, and nothing is scattered back (the three
    shapes differ from A's).  A replicated stack is computed on its holder.

``info`` of every ``gesvj`` stays on the device until the end of the
evaluation (``eigh._raise_on_info``'s one min-reduction and host read); a -1
raises ``np.linalg.LinAlgError('SVD did not converge')`` on every rank.

The three results hang off one ``SvdExpr`` node: forcing any runs the
computation once.
"""
import numpy as np

from .. import backend, comm, runtime
from ..array import distarray
from ..array import extent as ext
from ..array.blocks import gather_slabs, spans, whole, with_tiles
from ..array.views import transpose_of
from .base import Expr, as_array

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


class SvdTriple:
  """The value of an ``SvdExpr``: the arrays U, s, Vt (U and Vt None when only
  the singular values were asked for); shape and dtype: A's."""

  def __init__(self, U, s, Vt, shape, dtype):
    self.U, self.s, self.Vt = U, s, Vt
    self.shape, self.dtype = tuple(shape), np.dtype(dtype)


class SvdExpr(Expr):
  _members = ('array',)

  def compute_shape(self):
    return self.array.shape

  def compute_dtype(self):
    return np.dtype(self.array.dtype)

  def pretty_str(self):
    return 'Svd[%d](%s, compute_uv=%s)' % (self.expr_id, self.array, self.compute_uv)

  def _evaluate(self, deps):
    arr = distarray.as_array(deps['array'])
    return SvdTriple(*svd_array(arr, self.compute_uv), shape=arr.shape, dtype=arr.dtype)


class SvdPartExpr(Expr):
  """U (``part`` 0), s (1) or Vt (2) of an ``SvdExpr``."""
  _members = ('triple',)

  def compute_shape(self):
    s = tuple(self.triple.shape)
    lead, (m, n) = s[:-2], s[-2:]
    k = min(m, n)
    return lead + ((m, k), (k,), (k, n))[self.part]

  def compute_dtype(self):
    return np.dtype(self.triple.dtype)

  def pretty_str(self):
    return '%s(%s)' % (('U', 's', 'Vt')[self.part], self.triple)

  def _evaluate(self, deps):
    t = deps['triple']
    return (t.U, t.s, t.Vt)[self.part]


def _limits(dt, m, n):
  """(short side, long side, direct limit of the long side)."""
  k, long_side = min(m, n), max(m, n)
  return k, long_side, backend.gesvj_plan(dt, k)[1]


def svd(A, full_matrices=False, compute_uv=True):
  """``(U, s, Vt)``, lazily: the reduced singular value decomposition of the
  float32 / float64 matrix ``A`` of shape (m, n), or of every matrix of a stack
  (B, m, n); with ``compute_uv`` false the lazy ``s`` alone.  Evaluation raises
  ``np.linalg.LinAlgError`` for a matrix that holds a non-finite value or does
  not converge."""
  from .sparse import is_sparse
  if full_matrices:
    raise NotImplementedError('svd: full_matrices=True is not built; the reduced factors (full_matrices=False) are')
  if is_sparse(A):
    raise TypeError('svd: a sparse operand is not supported: convert it with todense() first')
  A = as_array(A)
  shape = tuple(A.shape)
  if len(shape) not in (2, 3):
    raise ValueError('svd: a matrix (m, n) or a stack (B, m, n) is needed, got shape %s' % (shape,))
  dt = np.dtype(A.dtype)
  if dt not in _FLOATS:
    raise TypeError('svd: dtype %s is not float32 / float64' % dt)
  m, n = shape[-2:]
  k, long_side, mmax = _limits(dt, m, n)
  nmax = backend.gesvj_plan(dt, 0)[0]
  if len(shape) == 3:
    if k > nmax or long_side > mmax:
      raise NotImplementedError('svd: a stack of %s matrices is above the limit of one workgroup for %s (the short '
                                'side at most %d, the long side at most %d beside it)' % ((m, n), dt, nmax, mmax))
  elif k > nmax or long_side > mmax:
    qmax = backend.geqr_plan(dt, k)[0]
    if k > min(nmax, qmax):
      raise NotImplementedError('svd: min(m, n) = %d is above the limits of %d (svd) and %d (qr) for %s'
                                % (k, nmax, qmax, dt))
  node = SvdExpr(array=A)
  node.compute_uv = bool(compute_uv)
  parts = []
  for part in (0, 1, 2):
    e = SvdPartExpr(triple=node)
    e.part = part
    parts.append(e)
  return tuple(parts) if compute_uv else parts[1]


def svdvals(A):
  """The singular values of ``svd(A)``, descending, lazily."""
  return svd(A, compute_uv=False)


def pinv(A, rcond=None):
  """The Moore-Penrose pseudo-inverse of the 2-d float32 / float64 ``A``,
  lazily: V diag(1 / s_j where s_j > rcond s_max, else 0) U^T, ``rcond``
  defaulting to max(m, n) eps(dtype).  Built as transpose(dot(U * inv_s, Vt)),
  so a tall A never leaves its owners."""
  from .builtins import astype, maximum
  from .dot import dot
  from .transpose import transpose
  A = as_array(A)
  if len(A.shape) != 2:
    raise ValueError('pinv: a 2-d array is needed, got shape %s' % (tuple(A.shape),))
  U, s, Vt = svd(A)
  dt = np.dtype(A.dtype)
  if rcond is None:
    rcond = max(A.shape) * float(np.finfo(dt).eps)
  cut = s[0:1] * dt.type(rcond)  # s is descending: s_max first
  # 1 / s_j where s_j is above the cut, else 0 (the quotient's floor keeps it finite where it is masked)
  inv_s = astype(s > cut, dt) * (dt.type(1) / maximum(s, np.finfo(dt).tiny))
  return transpose(dot(U * inv_s, Vt))


# ------------------------------------------------------------- evaluation
def _raise_on_info(infos):
  """``eigh._raise_on_info`` with this module's message.  Collective."""
  import torch
  ctx = runtime.get()
  worst = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
  for info in infos:
    if info.numel():
      worst = torch.minimum(worst, info.to(torch.int64).min().reshape(1))
  worst = comm.all_reduce(worst, 'min')
  if int(worst.item()) < 0:
    raise np.linalg.LinAlgError('SVD did not converge')


def _t(t):
  """The last two axes of the device block ``t`` swapped, contiguous."""
  return backend.get().contiguous(t.transpose(-1, -2))


def _block(t, compute_uv, infos):
  """(U, s, Vt) of the device block ``t`` (.., m, n), any orientation; its info
  joins ``infos``.  A wide block is solved transposed and the factors swapped."""
  be = backend.get()
  wide = t.shape[-2] < t.shape[-1]
  U, s, Vt, info = be.gesvj(_t(t) if wide else be.contiguous(t), compute_uv)
  infos.append(info)
  if wide and compute_uv:
    U, Vt = _t(Vt), _t(U)
  return U, s, Vt


def _rep(t):
  return None if t is None else distarray.ReplicatedArray(t)


def _tall(arr, compute_uv, infos):
  """The tall route: (U tiled like qr_array's Q, s, Vt replicated)."""
  import torch
  from .dot import run_dot
  from .qr import qr_array
  ctx = runtime.get()
  be = backend.get()
  Q, R = qr_array(arr)
  UR, s, Vt = _block(R.device_data(), compute_uv, infos)  # the same bits on every rank
  if not compute_uv:
    return None, _rep(s), None
  if Q.replicated:
    U = torch.empty_like(Q.device_data())
    be.gemm(be.contiguous(Q.device_data()), UR, U)
    return _rep(U), _rep(s), _rep(Vt)
  if spans(Q, (1,)):  # whole rows on their owners: no exchange
    local = {}
    for e, w in Q.tiles.items():
      if ctx.is_local(w):
        q = be.contiguous(Q.fetch(e))
        local[e] = torch.empty_like(q)
        if q.numel():
          be.gemm(q, UR, local[e])
    return distarray.from_tiles(Q.shape, Q.dtype, Q.tiles, local), _rep(s), _rep(Vt)
  return run_dot(Q, _rep(UR), None), _rep(s), _rep(Vt)


def _stack(arr, compute_uv, infos):
  """The 3-d route: U, s, Vt tiled along axis 0 at the slab cuts."""
  ctx = runtime.get()
  dt = np.dtype(arr.dtype)
  nb, m, n = arr.shape
  k = min(m, n)
  if spans(arr, (1, 2)):
    slabs = sorted(arr.tiles.items(), key=lambda kv: kv[0].ul[0])
    got = {qi: arr.fetch(e) for qi, (e, w) in enumerate(slabs) if ctx.is_local(w)}
  else:
    slabs, got = gather_slabs(arr, 0)
  shapes = ((nb, m, k), (nb, k), (nb, k, n))

  def cut(e, shape):
    return ext.create((e.ul[0],) + (0,) * (len(shape) - 1), (e.lr[0],) + tuple(shape[1:]), shape)

  tiles = [{cut(e, sh): w for e, w in slabs} for sh in shapes]
  local = [{}, {}, {}]
  for qi, t in got.items():
    for part, res in enumerate(_block(t, compute_uv, infos)):
      if res is not None:
        local[part][cut(slabs[qi][0], shapes[part])] = res
  return [distarray.from_tiles(shapes[p], dt, tiles[p], local[p]) if compute_uv or p == 1 else None
          for p in range(3)]


def svd_array(arr, compute_uv=True):
  """(U, s, Vt) arrays of the array ``arr`` (U and Vt None without
  ``compute_uv``)."""
  arr = with_tiles(arr)
  dt = np.dtype(arr.dtype)
  infos = []
  _, long_side, mmax = _limits(dt, *arr.shape[-2:])
  if long_side <= mmax and (arr.replicated or arr.ndim == 2):
    # held in full by every rank, or brought there by ONE exchange: the same bits everywhere
    out = _block(arr.device_data() if arr.replicated else whole(arr), compute_uv, infos)
    _raise_on_info(infos)
    return tuple(_rep(t) for t in out)
  if arr.ndim == 3:
    out = _stack(arr, compute_uv, infos)
    _raise_on_info(infos)
    return tuple(out)
  m, n = arr.shape
  if m >= n:
    U, s, Vt = _tall(arr, compute_uv, infos)
  else:  # the transposed problem, the factors swapped
    if arr.replicated:
      Ut, s, Vtt = _tall(_rep(_t(arr.device_data())), compute_uv, infos)
    else:
      Ut, s, Vtt = _tall(transpose_of(arr), compute_uv, infos)
    U = Vt = None
    if compute_uv:
      U = _rep(_t(Vtt.device_data()))
      Vt = _rep(_t(Ut.device_data())) if Ut.replicated else transpose_of(Ut)
  _raise_on_info(infos)
  return U, s, Vt

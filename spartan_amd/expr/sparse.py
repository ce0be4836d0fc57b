"""Sparse expressions: ``sparse_rand`` / ``sparse_diagonal`` / ``sparse_empty``,
sparse ``dot``, ``todense``, ``sum`` and scaling (the
reference's spartan/expr/builtins.py sparse constructors and the sparse
branches of spartan/expr/dot.py:51, :207-231).

A sparse expression is a node whose value is a ``SparseDistArray`` (row slabs
of CSR, array/sparse.py); the class mixin ``SparseExpr`` marks it.  What may
be done with one:

  * ``dot(S, X)``, X dense (n,), (n, 1) or (n, p): X is brought in full to
    every rank by ``blocks.whole`` (one ``gather_regions``; every rank issues
    it, with or without slabs), then each rank runs ``csrmm`` on each of its
    slabs.  The result is
    dense, in row slabs aligned with S's on the same workers; no cross-rank
    reduction.  One ``g`` (lanes per row) is taken from the whole matrix's
    plan and given to every slab, so a row's bits do not depend on the layout;
  * ``todense(S)``: ``csr_todense`` per slab, same slabs;
  * ``sum(S, axis=1 | None)``: ``dot`` with a ones vector, then the dense
    reduce; ``axis=0`` refuses: it is ``sum(sparse_transpose(S), axis=1)``;
  * ``S * c``, ``c * S``: the same structure with scaled values;
  * ``sparse_transpose(S)``: the transpose under its own name,
    ``SparseDistArray.transposed``.

Everything else refuses a sparse operand with a ``TypeError`` that names
``todense()`` -- at construction where the operand is visibly sparse, and in
``Expr.evaluate`` before any node body runs otherwise.  Nothing densifies
silently.
"""
import numpy as np

from .. import backend, runtime
from ..array import distarray
from ..array import extent as ext
from ..array import sparse as sparray
from ..array.blocks import whole
from ..array.sparse import TODENSE
from .base import Expr, Val

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _refuse(*_a, **_k):
  raise TypeError(TODENSE)


def _scalar(c):
  return isinstance(c, (int, float, np.integer, np.floating)) and not isinstance(c, (bool, np.bool_))


class SparseExpr(Expr):
  """Mixin of every node whose value is a SparseDistArray."""
  sparse_result = True
  accepts_sparse = True

  def __mul__(self, o):
    if not _scalar(o):
      _refuse()
    return SparseScaleExpr(array=self, scalar=o)

  __rmul__ = __mul__
  __add__ = __radd__ = __sub__ = __rsub__ = __truediv__ = __rtruediv__ = __floordiv__ = __rfloordiv__ = _refuse
  __mod__ = __pow__ = __neg__ = __lt__ = __gt__ = __le__ = __ge__ = __and__ = __or__ = __xor__ = _refuse
  __getitem__ = reshape = outer = mean = astype = argmin = argmax = _refuse
  __hash__ = Expr.__hash__

  def __eq__(self, o):
    _refuse()

  def __ne__(self, o):
    _refuse()

  @property
  def T(self):
    _refuse()

  def todense(self):
    return todense(self)

  def sum(self, axis=None):
    return sparse_sum(self, axis)


class SparseVal(SparseExpr, Val):
  """A forced SparseDistArray as an expression."""

  def pretty_str(self):
    return 'SparseVal(%s)' % (self.val,)


class SparseBuildExpr(SparseExpr):
  """A sparse array built at evaluation by ``self.build()``."""
  _members = ()

  def compute_shape(self):
    return self.build_shape

  def compute_dtype(self):
    return self.build_dtype

  def visit(self, visitor):
    return self

  def pretty_str(self):
    return '%s[%d]%s' % (self.what, self.expr_id, self.build_shape)

  def _evaluate(self, deps):
    return self.build()


def _build(what, shape, dtype, build):
  shape = tuple(int(s) for s in shape)
  dt = np.dtype(dtype)
  if len(shape) != 2:
    raise ValueError('%s: a 2-d shape is needed, got %s' % (what, shape))
  if dt not in _FLOATS:
    raise TypeError('%s: dtype %s is not float32 / float64' % (what, dt))
  e = SparseBuildExpr()
  e.what, e.build_shape, e.build_dtype, e.build = what, shape, dt, build
  return e


class SparseScaleExpr(SparseExpr):
  _members = ('array',)

  def compute_shape(self):
    return self.array.shape

  def compute_dtype(self):
    return np.dtype(self.array.dtype)

  def pretty_str(self):
    return 'Scale[%d](%s, %r)' % (self.expr_id, self.array, self.scalar)

  def _evaluate(self, deps):
    import torch
    from .. import codegen
    S = deps['array']
    be = backend.get()
    dt = np.dtype(S.dtype)
    root = codegen.Op('multiply', [codegen.In(0, dt), codegen.Sc(0, self.scalar)])
    if root.dtype != dt:
      root = codegen.Cast(root, dt)

    def scaled(v):
      out = torch.empty_like(v)
      be.map(root, {0: v}, out)
      return out
    return S.with_values(scaled)


class SparseTransposeExpr(SparseExpr):
  _members = ('array',)

  def compute_shape(self):
    return tuple(self.array.shape[::-1])

  def compute_dtype(self):
    return np.dtype(self.array.dtype)

  def pretty_str(self):
    return 'SparseTranspose[%d](%s)' % (self.expr_id, self.array)

  def _evaluate(self, deps):
    return sparray.transposed(deps['array'], self.tile_hint)


class ToDenseExpr(Expr):
  _members = ('array',)
  accepts_sparse = True

  def compute_shape(self):
    return self.array.shape

  def compute_dtype(self):
    return np.dtype(self.array.dtype)

  def pretty_str(self):
    return 'ToDense[%d](%s)' % (self.expr_id, self.array)

  def _evaluate(self, deps):
    return todense_array(deps['array'])


def is_sparse(x):
  """True for a sparse expression, a SparseDistArray or a scipy.sparse matrix."""
  return bool(getattr(x, 'sparse_result', False) or getattr(x, 'sparse', False)) or sparray.is_scipy_sparse(x)


def as_sparse_expr(x, tile_hint=None):
  """The sparse expression of a sparse expression, a SparseDistArray or a
  scipy.sparse matrix (ingested through ``from_scipy``)."""
  if isinstance(x, SparseExpr):
    return x
  if isinstance(x, sparray.SparseDistArray):
    return SparseVal(val=x)
  if sparray.is_scipy_sparse(x):
    return SparseVal(val=sparray.from_scipy(x, tile_hint))
  raise TypeError('a sparse array is needed, got %s' % type(x).__name__)


# ------------------------------------------------------------ constructors
def sparse_rand(shape, density=0.001, format='csr', dtype=np.float32, tile_hint=None, seed=None):
  """A random sparse array: the entries of ``scipy.sparse.random(m, n, density,
  dtype=dtype, random_state=np.random.RandomState(seed))``.  Every rank draws
  the whole matrix on the host and keeps its slabs (ingest, not a hot path), so
  the same seed gives the same array on every tile layout.  ``format`` is
  accepted for signature parity: storage is always CSR."""
  from .builtins import _new_seed
  seed = _new_seed(seed) % (2 ** 32)
  m, n = (int(s) for s in shape)
  dt = np.dtype(dtype)

  def build():
    import scipy.sparse as sp
    mat = sp.random(m, n, density=density, format='csr', dtype=dt, random_state=np.random.RandomState(seed))
    return sparray.from_scipy(mat, tile_hint)
  return _build('sparse_rand', (m, n), dt, build)


def sparse_diagonal(shape, dtype=np.float32, tile_hint=None):
  """Ones on the main diagonal of a (possibly rectangular) sparse array."""
  return _build('sparse_diagonal', shape, dtype, lambda: sparray.diagonal(shape, dtype, tile_hint))


def sparse_empty(shape, dtype=np.float32, tile_hint=None):
  """A sparse array without stored entries."""
  return _build('sparse_empty', shape, dtype, lambda: sparray.empty(shape, dtype, tile_hint))


# -------------------------------------------------------------- evaluation
def _out_extent(e, out_shape):
  if len(out_shape) == 1:
    return ext.create((e.ul[0],), (e.lr[0],), out_shape)
  return ext.create((e.ul[0], 0), (e.lr[0], out_shape[1]), out_shape)


def sparse_dot(S, x):
  """``S @ x`` for the SparseDistArray ``S`` (m, n) and the dense array ``x``
  (n,), (n, 1) or (n, p).  Collective: one gather of x to every rank."""
  import torch
  if getattr(x, 'sparse', False):
    raise TypeError('dot(sparse, sparse) is not supported: ' + TODENSE)
  ctx = runtime.get()
  be = backend.get()
  m, n = S.shape
  xs = tuple(x.shape)
  if len(xs) not in (1, 2) or xs[0] != n:
    raise ValueError('objects are not aligned')
  p = 1 if len(xs) == 1 else xs[1]
  out_shape = (m,) if len(xs) == 1 else (m, p)
  dt = np.dtype(np.result_type(S.dtype, x.dtype))
  if dt not in _FLOATS:
    raise TypeError('dot(sparse, dense): result dtype %s is not float32 / float64' % dt)
  X = be.contiguous(whole(x), dt).reshape(n, p)
  Sd = S.astype(dt)
  g = backend.csrmm_plan(dt, m, S.nnz, p)[0]  # one g for every slab: the layout does not change a row's bits
  tiles, local = {}, {}
  for e, w in S.tiles.items():
    d = _out_extent(e, out_shape)
    tiles[d] = w
    if e in S.local:
      t, td = S.local[e], Sd.local[e]
      C = torch.empty((e.shape[0], p), dtype=backend.torch_dtype(dt), device=ctx.device)
      # the analysis depends on rowptr alone: the tile of S keeps it, whatever dtype the values were cast to
      be.csrmm(t.rowptr, t.col, td.val, n, X, C, 1.0, 0.0, g, t.workspace)
      local[d] = C.reshape(d.shape)
  return distarray.from_tiles(out_shape, dt, tiles, local)


def sparse_als_solve(S, y, lam):
  """One ALS half-step on arrays: (X, infos) with X[i] the solution of row i of
  the SparseDistArray ``S`` (m, n) against the dense factor ``y`` (n, f) --
  ``als_solve`` on every local slab with ``y`` brought whole to every rank, as
  ``sparse_dot`` brings its right operand.  X is dense, (m, f), of S's dtype, in
  row slabs aligned with S's on the same workers; ``infos`` are the slabs'
  one-element device counters of failed rows, unread.  Collective: one gather
  of y; no cross-rank reduction."""
  import torch
  if getattr(y, 'sparse', False):
    raise TypeError('als: the factor is dense: ' + TODENSE)
  ctx = runtime.get()
  be = backend.get()
  m, n = S.shape
  if len(y.shape) != 2 or y.shape[0] != n:
    raise ValueError('als: a factor of %d rows is needed, got shape %s' % (n, tuple(y.shape)))
  f = int(y.shape[1])
  dt = np.dtype(S.dtype)
  Y = be.contiguous(whole(y), dt).reshape(n, f)
  tiles, local, infos = {}, {}, []
  for e, w in S.tiles.items():
    d = _out_extent(e, (m, f))
    tiles[d] = w
    if e in S.local:
      t = S.local[e]
      X = torch.empty((e.shape[0], f), dtype=backend.torch_dtype(dt), device=ctx.device)
      infos.append(be.als_solve(t.rowptr, t.col, t.val, n, Y, lam, X))
      local[d] = X
  return distarray.from_tiles((m, f), dt, tiles, local), infos


def todense_array(S):
  import torch
  if not getattr(S, 'sparse', False):
    return S
  ctx = runtime.get()
  be = backend.get()
  local = {}
  for e, t in S.local.items():
    D = torch.empty(e.shape, dtype=backend.torch_dtype(S.dtype), device=ctx.device)
    be.csr_todense(t.rowptr, t.col, t.val, S.shape[1], D)
    local[e] = D
  return distarray.from_tiles(S.shape, S.dtype, S.tiles, local)


def todense(S):
  """The dense array of a sparse one, in the same row slabs."""
  return ToDenseExpr(array=as_sparse_expr(S))


def sparse_transpose(S, tile_hint=None):
  """The transpose of a sparse array as a sparse expression of shape (n, m), in
  the row slabs of ``tile_hint`` (default: the rows dealt evenly to the
  workers).  ``glom()`` of it is scipy's ``A.T.tocsr()`` with sorted indices,
  bit for bit; explicit zeros are kept.  This is the one way to the transpose:
  ``S.T``, ``transpose(S)``, ``dot(dense, S)`` and ``sum(S, axis=0)`` still refuse.
  Column sums are ``sum(sparse_transpose(S), axis=1)``, and ``X @ S`` is
  ``transpose(dot(sparse_transpose(S), transpose(X)))``."""
  S = as_sparse_expr(S)
  if tile_hint is not None:
    tile_hint = tuple(int(h) for h in tile_hint)
    if len(tile_hint) != 2:
      raise ValueError('tile_hint %s does not match the 2-d shape %s' % (tile_hint, tuple(S.shape[::-1])))
    if tile_hint[1] < S.shape[0]:
      raise NotImplementedError('tile_hint %s cuts axis 1: sparse arrays are tiled in row slabs, every tile '
                                'spanning all %d columns (column-cut tilings are out of scope)'
                                % (tile_hint, S.shape[0]))
  return SparseTransposeExpr(array=S, tile_hint=tile_hint)


def sparse_sum(S, axis=None):
  """``sum`` of a sparse array along axis 1 or over everything: ``csrmm``
  against a ones vector, then (axis None) the dense reduce."""
  from .builtins import sum as dense_sum
  from .dot import dot
  S = as_sparse_expr(S)
  if axis == 0:
    raise NotImplementedError('sum(sparse, axis=0) needs the transpose, which is not built: use todense()')
  if axis not in (None, 1, -1):
    raise ValueError('sum(sparse): axis %r is out of range for a 2-d array' % (axis,))
  rows = dot(S, np.ones(S.shape[1], dtype=S.dtype))
  return rows if axis is not None else dense_sum(rows)

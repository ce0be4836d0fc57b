"""Sparse (CSR) distributed arrays.

The reference keeps a scipy.sparse matrix in a tile (``sparse=True``,
spartan/array/tile.pyx) and branches on it in ``dot`` (spartan/expr/dot.py:51,
:207-231).  Here a ``SparseDistArray`` is a 2-d float32 / float64 matrix in ROW
SLABS: every tile spans all columns, so a row is never split and a sparse x
dense product needs no cross-rank reduction.  A local tile holds three device
tensors -- ``rowptr`` (int64, tile-local row numbers), ``col`` (int32, global
column numbers), ``val`` -- and the cached structure analysis of ``csrmm``.
The array is immutable once built.

Every rank knows every slab's nonzero count (``slab_nnz``): the builders here
have it for free, and it lets ``glom`` lay out its exchange.

scipy is imported inside the functions that need it: importing this module
does not require it.
"""
import numpy as np

from .. import backend, comm, runtime
from . import distarray
from . import extent as ext
from . import transfer

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
TODENSE = 'a sparse array is not accepted here: convert it with todense() first'


def is_scipy_sparse(x):
  """True for a scipy.sparse matrix / array, without importing scipy."""
  mod = type(x).__module__ or ''
  return mod.startswith('scipy.sparse') and hasattr(x, 'tocsr')


class SparseTile:
  """One row slab on its owner: CSR with tile-local rows and global columns."""
  __slots__ = ('ex', 'rowptr', 'col', 'val', 'workspace')

  def __init__(self, ex, rowptr, col, val):
    self.ex, self.rowptr, self.col, self.val = ex, rowptr, col, val
    self.workspace = backend.CsrWorkspace()

  @property
  def nnz(self):
    return int(self.col.numel())


class SparseDistArray(distarray.DistArray):
  sparse = True

  def __init__(self, shape, dtype, tiles, local, slab_nnz=None):
    self.shape = tuple(int(s) for s in shape)
    self.dtype = np.dtype(dtype)
    if len(self.shape) != 2:
      raise ValueError('a sparse array is 2-d, got shape %s' % (self.shape,))
    if self.dtype not in _FLOATS:
      raise TypeError('sparse arrays hold float32 / float64, not %s (integer values are out of scope)' % self.dtype)
    for e in tiles:
      if e.ul[1] != 0 or e.lr[1] != self.shape[1]:
        raise NotImplementedError('sparse arrays are tiled in row slabs: tile %s cuts axis 1' % (e,))
    self.tiles = dict(tiles)     # {TileExtent: worker}, identical on every rank
    self.local = dict(local)     # {TileExtent: SparseTile} of this rank
    self.slab_nnz = dict(slab_nnz) if slab_nnz is not None else None
    self._nnz = None
    self.bad_tiles = []

  def slabs(self):
    """[(extent, worker)] in row order."""
    return sorted(self.tiles.items(), key=lambda kv: kv[0].ul[0])

  def _counts(self):
    """{extent: nonzeros} of every slab.  Collective when the builder did not
    supply it: one all-reduce of the per-slab counts."""
    if self.slab_nnz is None:
      import torch
      ctx = runtime.get()
      order = [e for e, _ in self.slabs()]
      cnt = torch.zeros((len(order),), dtype=torch.int64, device=ctx.device)
      for i, e in enumerate(order):
        if e in self.local:
          cnt[i] = self.local[e].nnz
      if ctx.distributed:
        comm.all_reduce(cnt, 'sum')
      self.slab_nnz = {e: int(c) for e, c in zip(order, cnt.cpu().tolist())}
    return self.slab_nnz

  @property
  def nnz(self):
    """The total number of stored entries (collective on first use, cached)."""
    if self._nnz is None:
      self._nnz = sum(self._counts().values())
    return self._nnz

  def real_size(self):
    return self.nnz

  def tile_shape(self):
    return max((e.shape for e in self.tiles), key=lambda s: s[0])

  def fetch(self, region):
    raise TypeError(TODENSE)

  def select(self, idx):
    raise TypeError(TODENSE)

  def update(self, region, data, reducer=None):
    raise TypeError('a sparse array is immutable once built')

  def with_values(self, fn, dtype=None):
    """The same structure with every local tile's values ``fn(val)``."""
    local = {e: SparseTile(e, t.rowptr, t.col, fn(t.val)) for e, t in self.local.items()}
    out = SparseDistArray(self.shape, dtype or self.dtype, self.tiles, local, self.slab_nnz)
    out._nnz = self._nnz
    return out

  def astype(self, dtype):
    dt = np.dtype(dtype)
    if dt == self.dtype:
      return self
    be = backend.get()
    return self.with_values(lambda v: be.contiguous(v, dt), dt)

  def glom(self):
    """Collective: the whole matrix as a scipy.sparse.csr_matrix on every
    rank.  The values, the columns and the row pointers travel as three 1-d
    arrays tiled like the slabs: one exchange each."""
    import scipy.sparse as sp
    ctx = runtime.get()
    m, n = self.shape
    counts = self._counts()
    order = self.slabs()
    total = self.nnz
    ranks = range(ctx.world_size)

    def gathered(length, dtype, spans, pick):
      tiles, local = {}, {}
      for (e, w), (a, b) in zip(order, spans):
        if b > a:
          x = ext.create((a,), (b,), (length,))
          tiles[x] = w
          if e in self.local:
            local[x] = pick(self.local[e])
      arr = distarray.from_tiles((length,), dtype, tiles, local)
      got = distarray.gather_regions(arr, [(ext.from_shape((length,)), r) for r in ranks])
      return transfer.download(got[ctx.rank]).reshape(length)

    offs = np.concatenate([[0], np.cumsum([counts[e] for e, _ in order])]).astype(np.int64)
    ends = gathered(m, np.int64, [(e.ul[0], e.lr[0]) for e, _ in order], lambda t: t.rowptr[1:])
    indptr = np.zeros(m + 1, np.int64)
    for (e, _), o in zip(order, offs[:-1]):
      indptr[e.ul[0] + 1:e.lr[0] + 1] = ends[e.ul[0]:e.lr[0]] + o
    if total:
      spans = list(zip(offs[:-1].tolist(), offs[1:].tolist()))
      data = gathered(total, self.dtype, spans, lambda t: t.val)
      indices = gathered(total, np.int32, spans, lambda t: t.col)
    else:
      data, indices = np.zeros(0, self.dtype), np.zeros(0, np.int32)
    out = sp.csr_matrix((data, indices, indptr), shape=(m, n))
    out.has_sorted_indices = True
    return out

  def transposed(self, tile_hint=None):
    """Collective: the transpose as a new SparseDistArray (``transposed``)."""
    return transposed(self, tile_hint)


# ---------------------------------------------------------------- builders
def slab_extents(shape, tile_hint=None):
  """{extent: worker} of the row slabs of ``shape``: ``compute_extents`` along
  axis 0 with round-robin placement.  Without a hint the rows are dealt evenly
  to the workers."""
  ctx = runtime.get()
  m, n = (int(s) for s in shape)
  if tile_hint is None:
    rows = max(1, -(-m // ctx.num_workers))
  else:
    if len(tile_hint) != 2:
      raise ValueError('tile_hint %s does not match the 2-d shape %s' % (tile_hint, (m, n)))
    if int(tile_hint[1]) < n:
      raise NotImplementedError('tile_hint %s cuts axis 1: sparse arrays are tiled in row slabs, every tile '
                                'spanning all %d columns (column-cut tilings are out of scope)' % (tuple(tile_hint), n))
    rows = max(1, int(tile_hint[0]))
  return distarray.compute_extents((m, n), (rows, n), ctx.num_workers)


def _up(a, dtype):
  import torch
  ctx = runtime.get()
  a = np.ascontiguousarray(a, dtype=dtype)
  if a.size == 0:
    return torch.empty((0,), dtype=backend.torch_dtype(dtype), device=ctx.device)
  return transfer.upload(a, ctx.device)


def from_csr_pieces(shape, dtype, tile_hint, piece, counts):
  """SparseDistArray whose slab (r0, r1) is ``piece(r0, r1)`` -> host (rowptr,
  col, val), asked only for this rank's slabs; ``counts(r0, r1)`` the slab's
  nonzero count (asked for every slab)."""
  ctx = runtime.get()
  shape = tuple(int(s) for s in shape)
  if len(shape) != 2:
    raise ValueError('a sparse array is 2-d, got shape %s' % (shape,))
  if np.dtype(dtype) not in _FLOATS:
    raise TypeError('sparse arrays hold float32 / float64, not %s (integer values are out of scope)' % np.dtype(dtype))
  if shape[1] > 2 ** 31 - 1:
    raise NotImplementedError('%d columns are outside the int32 column range' % shape[1])
  tiles = slab_extents(shape, tile_hint)
  local, nnz = {}, {}
  for e, w in tiles.items():
    r0, r1 = e.ul[0], e.lr[0]
    nnz[e] = int(counts(r0, r1))
    if ctx.is_local(w):
      rowptr, col, val = piece(r0, r1)
      local[e] = SparseTile(e, _up(rowptr, np.int64), _up(col, np.int32), _up(val, dtype))
  return SparseDistArray(shape, dtype, tiles, local, nnz)


def canonical_csr(mat):
  """A private scipy CSR copy of ``mat`` (any scipy.sparse format) with summed
  duplicates and sorted indices; explicit zeros are kept."""
  import scipy.sparse as sp
  if not is_scipy_sparse(mat):
    raise TypeError('from_scipy: a scipy.sparse matrix is needed, got %s' % type(mat).__name__)
  csr = sp.csr_matrix(mat, copy=True)
  csr.sum_duplicates()
  csr.sort_indices()
  return csr


def from_scipy(mat, tile_hint=None):
  """Upload a scipy.sparse matrix of any format: canonical CSR on the host, and
  each rank uploads only its own slabs."""
  csr = canonical_csr(mat)
  dt = np.dtype(csr.dtype)
  if dt not in _FLOATS:
    raise TypeError('from_scipy: dtype %s is not float32 / float64 (integer values are out of scope)' % dt)
  ip = csr.indptr.astype(np.int64)

  def piece(r0, r1):
    a, b = ip[r0], ip[r1]
    return ip[r0:r1 + 1] - a, csr.indices[a:b], csr.data[a:b]

  return from_csr_pieces(csr.shape, dt, tile_hint, piece, lambda r0, r1: ip[r1] - ip[r0])


def diagonal(shape, dtype=np.float32, tile_hint=None):
  """Ones on the main diagonal of a possibly rectangular array; each slab is
  built on its owner."""
  m, n = (int(s) for s in shape)
  k = min(m, n)

  def count(r0, r1):
    return max(0, min(r1, k) - r0)

  def piece(r0, r1):
    c = count(r0, r1)
    rowptr = np.minimum(np.arange(r1 - r0 + 1, dtype=np.int64), c)
    return rowptr, np.arange(r0, r0 + c, dtype=np.int32), np.ones(c, dtype)

  return from_csr_pieces((m, n), np.dtype(dtype), tile_hint, piece, count)


def empty(shape, dtype=np.float32, tile_hint=None):
  """No stored entries."""
  def piece(r0, r1):
    return np.zeros(r1 - r0 + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype)

  return from_csr_pieces(shape, np.dtype(dtype), tile_hint, piece, lambda r0, r1: 0)


# --------------------------------------------------------------- transpose
def _through(be, src, perm):
  """``src[perm]`` for 1-d device tensors (``take``)."""
  import torch
  out = torch.empty_like(src)
  n = int(src.numel())
  be.take(src, perm, out, (1, n, 1), 0, n)
  return out


def _sorted_by_column(be, t, r0):
  """(col, row, val) of the tile ``t`` whose first row is ``r0``, ordered by
  (column, row): the entries are stored in row order and the sort is stable."""
  import torch
  nz = t.nnz
  rows = torch.empty((nz,), dtype=torch.int32, device=t.col.device)
  be.csr_rowids(t.rowptr, r0, rows)
  keys = torch.empty_like(t.col)
  perm = torch.empty((nz,), dtype=torch.int64, device=t.col.device)
  be.sort(t.col, keys, perm, (1, nz, 1))
  return keys, _through(be, rows, perm), _through(be, t.val, perm)


def _cuts(be, col, n, bounds):
  """Host int64 array: how many of the column numbers ``col`` lie below each
  of the ascending ``bounds`` (1 .. n) -- ``bincount``, an inclusive ``scan`` and
  a ``take`` of the counts at the bounds."""
  import torch
  per = torch.empty((n,), dtype=torch.int64, device=col.device)
  be.bincount(be.contiguous(col, np.int64), per)
  cum = torch.empty_like(per)
  be.scan(per, cum, (1, n, 1))
  at = _up(np.asarray(bounds, np.int64) - 1, np.int64)
  ends = torch.empty((len(bounds),), dtype=torch.int64, device=col.device)
  be.take(cum, at, ends, (1, n, 1), 0, n)
  return transfer.download(ends).reshape(-1).astype(np.int64)


def transposed(S, tile_hint=None):
  """Collective: ``S.T`` as a SparseDistArray of shape (n, m) in the row slabs
  of ``slab_extents((n, m), tile_hint)``.  Every row of the
  result has ascending columns, explicit zeros are kept, and neither the
  layout of ``S`` nor the worker count changes a bit of it.

  Each local slab orders its entries by (column, row) with the stable radix
  sort, cuts them at the row bounds of the target slabs and sends every piece
  to the target's owner: one ``gather_regions`` for each of the three arrays
  (old column, old row, value).  A target concatenates its pieces in source
  order -- row order -- and, when there is more than one source slab, sorts
  them once more, stably, by the old column.  The per-piece counts reach every
  rank in one all-reduce; they lay out the exchange and give ``slab_nnz``."""
  import torch
  from .. import codegen
  ctx = runtime.get()
  be = backend.get()
  m, n = S.shape
  if m > 2 ** 31 - 1:
    raise NotImplementedError('%d rows are outside the int32 column range of the transpose' % m)
  tiles = slab_extents((n, m), tile_hint)
  src = S.slabs()
  dst = sorted(tiles.items(), key=lambda kv: kv[0].ul[0])
  bounds = [e.lr[0] for e, _ in dst]

  # 1. every local slab in (column, row) order, and its cuts at the target bounds
  ordered = {}
  cnt = np.zeros((len(src), len(dst)), np.int64)
  for si, (e, _) in enumerate(src):
    if e in S.local and S.local[e].nnz:
      t = S.local[e]
      ordered[si] = _sorted_by_column(be, t, e.ul[0])
      cnt[si] = np.diff(np.concatenate([[0], _cuts(be, t.col, n, bounds)]))
  if ctx.distributed:
    dev = _up(cnt.reshape(-1), np.int64)
    comm.all_reduce(dev, 'sum')
    cnt = transfer.download(dev).reshape(cnt.shape).astype(np.int64)
  totals = cnt.sum(axis=0)
  total = int(totals.sum())
  slab_nnz = {e: int(c) for (e, _), c in zip(dst, totals)}

  # 2. one exchange per array: the pieces laid out by (target, source)
  got = [{}, {}, {}]
  if total:
    base = np.concatenate([[0], np.cumsum(totals)])
    requests = [(ext.create((int(base[j]),), (int(base[j + 1]),), (total,)), ctx.owner(w))
                for j, (_, w) in enumerate(dst) if totals[j]]
    asked = [j for j in range(len(dst)) if totals[j]]
    for which, dtype in ((0, np.int32), (1, np.int32), (2, S.dtype)):
      xt, xl = {}, {}
      for j in asked:
        at = int(base[j])
        for si, (_, w) in enumerate(src):
          c = int(cnt[si, j])
          if c:
            x = ext.create((at,), (at + c,), (total,))
            xt[x] = w
            if si in ordered:
              a = int(cnt[si, :j].sum())
              xl[x] = ordered[si][which][a:a + c]
            at += c
      arr = distarray.from_tiles((total,), dtype, xt, xl)
      res = distarray.gather_regions(arr, requests)
      got[which] = {asked[qi]: t for qi, t in res.items()}

  # 3. every local target slab: rows in order, columns ascending, a tile-local rowptr
  local = {}
  for j, (e, w) in enumerate(dst):
    if not ctx.is_local(w):
      continue
    rows = e.lr[0] - e.ul[0]
    if not totals[j]:
      local[e] = SparseTile(e, torch.zeros((rows + 1,), dtype=torch.int64, device=ctx.device),
                            _up(np.zeros(0), np.int32), _up(np.zeros(0), S.dtype))
      continue
    keys, col, val = (be.contiguous(got[which][j]).reshape(-1) for which in range(3))
    nz = int(keys.numel())
    if len(src) > 1:  # pieces of several slabs: row order within a piece, not across the pieces of one column
      perm = torch.empty((nz,), dtype=torch.int64, device=keys.device)
      be.sort(keys, None, perm, (1, nz, 1))
      col, val = _through(be, col, perm), _through(be, val, perm)
    rel = torch.empty((nz,), dtype=torch.int64, device=keys.device)
    be.map(codegen.Cast(codegen.Op('subtract', [codegen.In(0, np.int32), codegen.Sc(0, int(e.ul[0]))]), np.int64),
           {0: keys}, rel)
    per = torch.zeros((rows + 1,), dtype=torch.int64, device=keys.device)
    be.bincount(rel, per[:rows])
    rowptr = torch.empty_like(per)
    be.scan(per, rowptr, (1, rows + 1, 1), exclusive=True)
    local[e] = SparseTile(e, rowptr, col, val)
  return SparseDistArray((n, m), S.dtype, tiles, local, slab_nnz)

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

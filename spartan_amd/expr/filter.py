"""Indexing by arrays: ``take`` / ``compress`` and ``a[i]`` with ``i`` an
expression (the ground of spartan/expr/filter.py).

The contract is NumPy's.  The reference's integer path (filter.py:50-76: a
1-d index on axis 0) is ``np.take(a, idx, axis=0)`` and is kept, for any axis.
Its bool path (filter.py:79-97) returns a masked array of the input's size
with the mask sense inverted; that is NOT restated: ``a[mask]`` here is
NumPy's -- the selected elements in C order, 1-d -- and ``compress`` is
``np.compress``.

One node, ``FilterExpr(src, idx)``, with three modes:

  take      the shape is known without evaluation.  If every tile spans the
            axis, each tile is gathered on its owner (``spx_take``) with the
            whole index; the output keeps the input's layout on the other
            axes and nothing but the index moves.  Otherwise (``a[idx]`` on
            row strips) every rank zero-fills one buffer of the output's full
            shape, each local tile writes the rows it owns into it (the
            kernel skips the others), the buffer is summed over ranks as an
            integer view of its bits -- every position has one contributor,
            so the sum reproduces the bits, -0.0 included; bool goes through
            int32 -- and each rank cuts its tiles of a default-layout target
            out of it.  The output must therefore fit on one GPU; a
            reduce-scatter or point-to-point delivery is the follow-up.
  compress  (an integer axis) each tile compacts its own part of the axis
            with its slice of the condition (``spx_compact_count`` /
            ``spx_compact``); no array data is exchanged.  The per-split
            counts are summed over ranks and downloaded once; their cumsum
            moves the cuts along the axis to [base, base + count).  Splits
            that select nothing are dropped, so the output tiles are uneven.
  mask      ``a[mask]`` / ``compress(axis=None)``: the array is cut into
            slabs along axis 0 at its own tile boundaries; each slab (a view
            when its tile spans the other axes, else gathered: one
            ``blocks.gather_slabs``) meets the matching region of the mask on one
            owner and is compacted flat into the run [base, base + count) of
            the 1-d result.

The shape of the last two depends on the data: ``compute_shape`` raises
``NotShapeable`` and ``.shape`` forces the node.  The index (or the 1-d
condition) is brought whole to every rank by one ``gather_regions``; every
rank issues the same collectives whether or not it owns tiles, and a rank
without tiles still range-checks the index, so an ``IndexError`` is raised
on every rank, when the node is forced and not before.  A result without
elements is a host array of the right shape and dtype (there are no empty
tiles).

Not supported: N-d or tuple-of-array indices, assignment through an index,
and a raw host array or list inside ``[]`` (``Expr.__getitem__`` refuses it
as before: pass host indices through ``take`` / ``compress`` or
``from_numpy``).
"""
import numpy as np

from .. import backend, comm, runtime
from ..array import distarray, transfer
from ..array import extent as ext
from ..array.blocks import axis_geom, gather_slabs, spans, whole, with_tiles
from ..util import prod
from .base import Expr, NotShapeable, as_array


class FilterExpr(Expr):
  _members = ('src', 'idx')

  def compute_shape(self):
    if self.mode != 'take':
      raise NotShapeable
    s = tuple(self.src.shape)
    return s[:self.axis] + (self.idx.shape[0],) + s[self.axis + 1:]

  def compute_dtype(self):
    return np.dtype(self.src.dtype)

  def pretty_str(self):
    return '%s[%d](%s, %s, axis=%s)' % (self.mode.capitalize(), self.expr_id, self.src, self.idx, self.axis)

  def _evaluate(self, deps):
    src, idx = distarray.as_array(deps['src']), distarray.as_array(deps['idx'])
    if self.mode == 'take':
      return take_array(src, idx, self.axis)
    if self.mode == 'compress' and self.axis is not None:
      return compress_array(src, idx, self.axis)
    return mask_array(src, idx, flat=self.mode == 'compress')


def _node(src, idx, mode, axis):
  e = FilterExpr(src=src, idx=idx)
  e.mode = mode
  e.axis = axis
  return e


def _axis(a, axis, name):
  nd = len(a.shape)
  if nd == 0:
    raise ValueError('%s: a 0-d array has no axis' % name)
  if not isinstance(axis, (int, np.integer)) or not -nd <= axis < nd:
    raise ValueError('%s: axis %r is out of range for a %d-d array' % (name, axis, nd))
  return int(axis) % nd


def _as_index(indices, name):
  """A 1-d int32 / int64 index expression."""
  if not isinstance(indices, Expr):
    host = np.asarray(indices)
    if host.size == 0 and host.ndim == 1:
      host = host.astype(np.int64)  # np.take accepts []
    indices = as_array(host)
  dt = np.dtype(indices.dtype)
  if dt.kind not in 'iu':
    raise IndexError('%s: arrays used as indices must be of integer type, not %s' % (name, dt))
  if len(indices.shape) != 1:
    raise NotImplementedError('%s: only 1-d index arrays have a gfx950 path (got %d-d)' % (name, len(indices.shape)))
  if dt not in (np.dtype(np.int32), np.dtype(np.int64)):
    indices = indices.astype(np.int64)
  return indices


def _as_condition(condition):
  """A bool expression: anything else goes through the ``!= 0`` map."""
  if not isinstance(condition, Expr):
    condition = as_array(np.asarray(condition))
  if np.dtype(condition.dtype) != np.bool_:
    condition = condition != 0
  return condition


def take(a, indices, axis=0):
  """``np.take(a, indices, axis)``, lazily: ``indices`` is a 1-d integer
  expression, array or list (negative values wrap).  An index outside
  [-n, n) raises IndexError when the node is forced."""
  a = as_array(a)
  return _node(a, _as_index(indices, 'take'), 'take', _axis(a, axis, 'take'))


def compress(condition, a, axis=None):
  """``np.compress(condition, a, axis)``, lazily: ``condition`` is 1-d; with
  ``axis=None`` it selects from the flattened array.  A condition shorter than
  the axis drops the tail; a longer one with a true element past the end
  raises IndexError when the node is forced."""
  a = as_array(a)
  condition = _as_condition(condition)
  if len(condition.shape) != 1:
    raise ValueError('compress: condition must be a 1-d array')
  if axis is None:
    if len(a.shape) == 0:
      raise ValueError('compress: a 0-d array has no axis')
    return _node(a, condition, 'compress', None)
  return _node(a, condition, 'compress', _axis(a, axis, 'compress'))


def getitem(a, i):
  """``a[i]`` for an expression ``i``: an integer index is ``take(a, i, 0)``;
  a bool one of a's shape gives the selected elements in C order, a 1-d one of
  length ``a.shape[0]`` is ``compress(i, a, 0)``."""
  dt = np.dtype(i.dtype)
  if dt == np.bool_:
    if len(a.shape) == 0:
      raise IndexError('a 0-d array cannot be indexed by a mask')
    if tuple(i.shape) == tuple(a.shape):
      return _node(a, i, 'mask', None)
    if len(i.shape) == 1 and i.shape[0] == a.shape[0]:
      return compress(i, a, 0)
    raise IndexError('boolean index of shape %s does not match the array of shape %s (the whole shape, or axis 0)'
                     % (tuple(i.shape), tuple(a.shape)))
  return take(a, i, 0)


# ------------------------------------------------------------- evaluation
def _empty(shape, dtype):
  return distarray.LocalWrapper(np.empty(tuple(shape), np.dtype(dtype)))


def _whole_1d(arr):
  """The 1-d array ``arr`` on every rank (``blocks.whole``), or None if it has
  no elements."""
  return whole(arr).reshape(-1) if arr.shape[0] else None


def _zeros(shape, tdt):
  import torch
  t = torch.empty(tuple(shape), dtype=tdt, device=runtime.get().device)
  if t.numel():
    backend.get().fill(t, backend.FILL_CONST, 0, 0, 0, (0,) * len(shape), tuple(shape))
  return t


def _fit(t, length):
  """The 1-d bool tensor ``t`` (or None) cut or zero-padded to ``length``."""
  be = backend.get()
  have = 0 if t is None else t.numel()
  if have == length:
    return be.contiguous(t)
  if have > length:
    return be.contiguous(t[:length])
  out = _zeros((length,), backend.torch_dtype(np.bool_))
  if have:
    be.copy_region(out, (0,), t, (0,), (have,))
  return out


def _bits_dtype(dtype):
  """The integer dtype an array of ``dtype`` is summed over ranks in."""
  dtype = np.dtype(dtype)
  return {1: np.dtype(np.bool_), 4: np.dtype(np.int32), 8: np.dtype(np.int64)}[dtype.itemsize]


def _take_into(buf, e, src, idx, axis, n):
  """The rows tile ``e`` owns, written into ``buf`` (the output's full shape)."""
  import torch
  be = backend.get()
  nd = len(buf.shape)
  m = buf.shape[axis]
  oshape = tuple(buf.shape)
  full = lambda d: e.ul[d] == 0 and e.lr[d] == e.array_shape[d]
  geom = axis_geom(e.shape, axis)
  if all(full(d) for d in range(1, axis)) and all(full(d) for d in range(axis + 2, nd)):
    # the tile's block of every output row is one run of the buffer: write in place
    after = prod(oshape[axis + 1:])
    off = (e.ul[0] * prod(oshape[1:]) if axis > 0 else 0) + \
          (e.ul[axis + 1] * prod(oshape[axis + 2:]) if axis + 1 < nd else 0)
    be.take(src, idx, buf.reshape(-1)[off:], geom, e.ul[axis], n, (m * after, after))
    return
  ul = tuple(0 if d == axis else e.ul[d] for d in range(nd))
  shape = tuple(m if d == axis else e.shape[d] for d in range(nd))
  tmp = torch.empty(shape, dtype=buf.dtype, device=buf.device)
  be.copy_region(tmp, (0,) * nd, buf, ul, shape)
  be.take(src, idx, tmp, geom, e.ul[axis], n)
  be.copy_region(buf, ul, tmp, (0,) * nd, shape)


def take_array(arr, ia, axis):
  import torch
  ctx = runtime.get()
  be = backend.get()
  arr = with_tiles(arr)
  backend.spx_dtype(arr.dtype)
  n, m = arr.shape[axis], ia.shape[0]
  oshape = tuple(arr.shape[:axis]) + (m,) + tuple(arr.shape[axis + 1:])
  if prod(oshape) == 0:
    return _empty(oshape, arr.dtype)
  idx = _whole_1d(ia)
  tdt = backend.torch_dtype(arr.dtype)
  if arr.replicated:
    out = torch.empty(oshape, dtype=tdt, device=ctx.device)
    be.take(be.contiguous(arr.device_data()), idx, out, axis_geom(arr.shape, axis), 0, n)
    return distarray.ReplicatedArray(out)
  local = [e for e, w in arr.tiles.items() if ctx.is_local(w)]
  if not local:  # no tile here: the index is range-checked all the same, so every rank raises
    be.take(torch.empty((0,), dtype=tdt, device=ctx.device), idx, torch.empty((m,), dtype=tdt, device=ctx.device),
            (1, 0, 1), 0, n)
  if spans(arr, (axis,)):
    tiles, out_local = {}, {}
    for e, w in arr.tiles.items():
      oe = ext.create(tuple(0 if d == axis else u for d, u in enumerate(e.ul)),
                      tuple(m if d == axis else l for d, l in enumerate(e.lr)), oshape)
      tiles[oe] = w
      if ctx.is_local(w):
        out = torch.empty(oe.shape, dtype=tdt, device=ctx.device)
        be.take(be.contiguous(arr.fetch(e)), idx, out, axis_geom(e.shape, axis), 0, n)
        out_local[oe] = out
    return distarray.from_tiles(oshape, arr.dtype, tiles, out_local)
  bdt = _bits_dtype(arr.dtype)
  tbdt = backend.torch_dtype(bdt)
  buf = _zeros(oshape, tbdt)
  for e in local:
    _take_into(buf, e, be.contiguous(arr.fetch(e)).view(tbdt), idx, axis, n)
  if bdt == np.bool_:
    buf = be.contiguous(buf, np.int32)
  comm.all_reduce(buf, 'sum')
  if bdt == np.bool_:
    buf = be.contiguous(buf, np.bool_)
  tiles = distarray.compute_extents(oshape, None, ctx.num_workers)
  out_local = {}
  for e, w in tiles.items():
    if ctx.is_local(w):
      piece = torch.empty(e.shape, dtype=buf.dtype, device=ctx.device)
      be.copy_region(piece, (0,) * len(oshape), buf, e.ul, e.shape)
      out_local[e] = piece.view(tdt)
  return distarray.from_tiles(oshape, arr.dtype, tiles, out_local)


def _sum_counts(counts):
  """Per-split counts (each split counted on one rank) summed over ranks: one
  collective and one download."""
  ctx = runtime.get()
  if not ctx.distributed:
    return counts
  t = transfer.upload(counts, ctx.device)
  comm.all_reduce(t, 'sum')
  return transfer.download(t).reshape(counts.shape)


def _tail_selected(cond, n):
  """Does the 1-d condition tensor select anything at or past ``n``?"""
  if cond is None or cond.numel() <= n:
    return False
  be = backend.get()
  return be.compact_count(be.contiguous(cond[n:]))[0] > 0


def compress_array(arr, ca, axis):
  import torch
  ctx = runtime.get()
  be = backend.get()
  arr = with_tiles(arr)
  backend.spx_dtype(arr.dtype)
  n = arr.shape[axis]
  cond = _whole_1d(ca)
  if _tail_selected(cond, n):
    raise IndexError('compress: the condition of length %d selects past an axis of length %d' % (ca.shape[0], n))
  cond = _fit(cond, n)
  tdt = backend.torch_dtype(arr.dtype)
  oshape = lambda c: tuple(arr.shape[:axis]) + (c,) + tuple(arr.shape[axis + 1:])
  if arr.replicated:
    total, ws = be.compact_count(cond)
    if total == 0:
      return _empty(oshape(0), arr.dtype)
    out = torch.empty(oshape(total), dtype=tdt, device=ctx.device)
    be.compact(be.contiguous(arr.device_data()), cond, out, axis_geom(arr.shape, axis), ws)
    return distarray.ReplicatedArray(out)
  cuts = sorted({(e.ul[axis], e.lr[axis]) for e in arr.tiles})
  sid = {lo: s for s, (lo, _) in enumerate(cuts)}
  first = {}  # split -> the rank that counts it for everyone
  for e, w in sorted(arr.tiles.items(), key=lambda kv: kv[0].ul):
    first.setdefault(sid[e.ul[axis]], ctx.owner(w))
  counts = np.zeros(len(cuts), np.int64)
  masks, wss = {}, {}
  for s in sorted({sid[e.ul[axis]] for e, w in arr.tiles.items() if ctx.is_local(w)}):
    lo, hi = cuts[s]
    masks[s] = be.contiguous(cond[lo:hi])
    c, wss[s] = be.compact_count(masks[s])
    if first[s] == ctx.rank:
      counts[s] = c
  counts = _sum_counts(counts)
  bases = np.concatenate(([0], np.cumsum(counts)))
  total = int(bases[-1])
  if total == 0:
    return _empty(oshape(0), arr.dtype)
  tiles, out_local = {}, {}
  for e, w in arr.tiles.items():
    s = sid[e.ul[axis]]
    c = int(counts[s])
    if c == 0:
      continue
    oe = ext.create(tuple(int(bases[s]) if d == axis else u for d, u in enumerate(e.ul)),
                    tuple(int(bases[s]) + c if d == axis else l for d, l in enumerate(e.lr)), oshape(total))
    tiles[oe] = w
    if ctx.is_local(w):
      out = torch.empty(oe.shape, dtype=tdt, device=ctx.device)
      be.compact(be.contiguous(arr.fetch(e)), masks[s], out, axis_geom(e.shape, axis), wss[s])
      out_local[oe] = out
  return distarray.from_tiles(oshape(total), arr.dtype, tiles, out_local)


def mask_array(arr, ma, flat):
  """``arr[ma]`` (``ma`` of arr's shape) or, with ``flat``, ``np.compress(ma,
  arr)`` for a 1-d ``ma`` over the flattened array."""
  import torch
  ctx = runtime.get()
  be = backend.get()
  arr = with_tiles(arr)
  backend.spx_dtype(arr.dtype)
  size = prod(arr.shape)
  tdt = backend.torch_dtype(arr.dtype)
  k = ma.shape[0] if flat else size
  if flat and k > size:
    tail = ext.create((size,), (k,), (k,))
    if ma.replicated:
      t = ma.fetch(tail)
    else:
      t = distarray.gather_regions(ma, [(tail, r) for r in range(ctx.world_size)])[ctx.rank]
    if be.compact_count(be.contiguous(t).reshape(-1))[0] > 0:
      raise IndexError('compress: the condition of length %d selects past the %d elements of the array' % (k, size))
    k = size
  if arr.replicated:
    cond = _fit(_whole_1d(ma), size) if flat else whole(ma).reshape(-1)
    total, ws = be.compact_count(cond)
    if total == 0:
      return _empty((0,), arr.dtype)
    out = torch.empty((total,), dtype=tdt, device=ctx.device)
    be.compact(be.contiguous(arr.device_data()).reshape(-1), cond, out, (1, size, 1), ws)
    return distarray.ReplicatedArray(out)
  slabs, got = gather_slabs(arr, 0)
  row = prod(arr.shape[1:])
  if flat:
    # the slab's flat run [a, b) of the condition, as far as the condition reaches
    runs = [(e.ul[0] * row, min(e.lr[0] * row, k)) for e, _ in slabs]
    reqs = [(qi, ext.create((a,), (b,), tuple(ma.shape))) for qi, (a, b) in enumerate(runs) if a < b]
    mgot = distarray.gather_regions(ma, [(r, ctx.owner(slabs[qi][1])) for qi, r in reqs])
    mgot = {reqs[j][0]: t for j, t in mgot.items()}
  else:
    mgot = distarray.gather_regions(ma, [(ext.create(e.ul, e.lr, tuple(ma.shape)), ctx.owner(w)) for e, w in slabs])
  counts = np.zeros(len(slabs), np.int64)
  conds, wss = {}, {}
  for qi, (e, w) in enumerate(slabs):
    if ctx.owner(w) != ctx.rank:
      continue
    t = mgot.get(qi)
    cond = _fit(None if t is None else be.contiguous(t).reshape(-1), e.size)
    conds[qi] = cond
    counts[qi], wss[qi] = be.compact_count(cond)
  counts = _sum_counts(counts)
  bases = np.concatenate(([0], np.cumsum(counts)))
  total = int(bases[-1])
  if total == 0:
    return _empty((0,), arr.dtype)
  tiles, out_local = {}, {}
  for qi, (e, w) in enumerate(slabs):
    c = int(counts[qi])
    if c == 0:
      continue
    oe = ext.create((int(bases[qi]),), (int(bases[qi]) + c,), (total,))
    tiles[oe] = w
    if ctx.owner(w) == ctx.rank:
      out = torch.empty((c,), dtype=tdt, device=ctx.device)
      be.compact(be.contiguous(got[qi]).reshape(-1), conds[qi], out, (1, e.size, 1), wss[qi])
      out_local[oe] = out
  return distarray.from_tiles((total,), arr.dtype, tiles, out_local)

"""``scan`` -- cumulative sum along an axis (restates spartan/expr/scan.py).

The reference computes per-tile totals with a shuffle (scan.py:24-38,
``_scan_reduce_mapper``), gloms and scans them on the master (:83-90) and
then maps every tile with its base added to the tile's first slice
(:42-64, ``_scan_mapper``).  Here the same three steps stay on the device:

  1. per-tile line totals by ``spx_scan``'s totals-only pass, written into a
     zero-initialised tensor in the ACCUMULATOR dtype (int64 / float64) whose
     shape is the array's with the scan axis replaced by T, the number of
     tile splits along it (``axis=None``: the last axis);
  2. the totals tensor is summed over ranks (the tiles are disjoint, so every
     position has one contributor and the sum is exact) and scanned
     exclusively on the device -- along the tile axis, or over the flattened
     tensor for ``axis=None`` (row-major order of (..., row, tile column) is
     the flat order of the row segments);
  3. each local tile is scanned with ``carry`` = its slice of the bases.

With T == 1 and an integer axis no tile needs a base and steps 1-2 are
skipped.  Every rank issues the same collective whether or not it owns
tiles.  Only ``(np.sum, np.cumsum)`` runs on the device; any other pair of
callables takes a host path that restates the reference literally (as
elsewhere, mappers that cannot be traced run on the host).

``axis=None`` keeps the reference's meaning, ``np.cumsum(a.ravel())`` in the
array's shape (tests/test_scan.py:4-5 there), for any number of dimensions
(the reference handles two).
"""
import numpy as np

from .. import backend, comm, runtime
from ..array import distarray, transfer
from ..array.blocks import axis_geom, with_tiles
from ..util import prod
from .base import Expr, as_array


class ScanExpr(Expr):
  _members = ('array',)

  def compute_shape(self):
    return self.array.shape

  def compute_dtype(self):
    dt = np.dtype(self.array.dtype)
    if self.reduce_fn is np.sum and self.scan_fn is np.cumsum:
      return backend.scan_dtypes(dt)[0]
    return np.asarray(self.scan_fn(np.zeros((1,) * max(1, len(self.array.shape)), dt), axis=self.axis)).dtype

  def pretty_str(self):
    return 'Scan[%d](%s, axis=%s)' % (self.expr_id, self.array, self.axis)

  def _evaluate(self, deps):
    arr = distarray.as_array(deps['array'])
    if self.reduce_fn is np.sum and self.scan_fn is np.cumsum:
      return scan_array(arr, self.axis)
    return scan_array_host(arr, self.reduce_fn, self.scan_fn, self.axis)


def scan(array, reduce_fn=np.sum, scan_fn=np.cumsum, axis=None):
  """Scan ``array`` over ``axis`` (default: the flattened array, in the
  array's shape) -- lazily; ``reduce_fn`` gives a tile's totals and
  ``scan_fn`` the scan itself (scan.py:67-96)."""
  array = as_array(array)
  nd = len(array.shape)
  if axis is not None:
    if not isinstance(axis, (int, np.integer)) or not -nd <= axis < nd:
      raise ValueError('scan: axis %r is out of range for a %d-d array' % (axis, nd))
    axis = int(axis) % nd
  elif nd == 0:
    raise ValueError('scan: a 0-d array has no axis to scan')
  e = ScanExpr(array=array)
  e.reduce_fn = reduce_fn
  e.scan_fn = scan_fn
  e.axis = axis
  return e


# ------------------------------------------------------------------ layout
def _axis_splits(arr, ax):
  """{ul[ax]: tile id along ax} of the array's tile grid."""
  cuts = sorted({(ex.ul[ax], ex.lr[ax]) for ex in arr.tiles})
  for (_, lr), (ul, _) in zip(cuts, cuts[1:]):
    if lr != ul:
      raise NotImplementedError('scan over a tile layout that is not a grid along axis %d' % ax)
  return {ul: i for i, (ul, _) in enumerate(cuts)}


def _bases_region(ex, ax, tid):
  ul = tuple(tid if d == ax else ex.ul[d] for d in range(ex.ndim))
  shape = tuple(1 if d == ax else ex.shape[d] for d in range(ex.ndim))
  return ul, shape


# ------------------------------------------------------------- device path
def scan_array(arr, axis):
  import torch
  ctx = runtime.get()
  be = backend.get()
  arr = with_tiles(arr)
  if arr.ndim == 0:
    raise ValueError('scan: a 0-d array has no axis to scan')
  odt, adt = backend.scan_dtypes(arr.dtype)
  nd = arr.ndim
  ax = nd - 1 if axis is None else axis
  if arr.replicated:  # one tile held in full by every rank
    src = be.contiguous(arr.device_data())
    out = torch.empty(arr.shape, dtype=backend.torch_dtype(odt), device=src.device)
    be.scan(src, out, (1, prod(arr.shape), 1) if axis is None else axis_geom(arr.shape, ax))
    return distarray.ReplicatedArray(out)
  tids = _axis_splits(arr, ax)
  T = len(tids)
  local = [ex for ex, w in arr.tiles.items() if ctx.is_local(w)]
  data = {ex: be.contiguous(arr.fetch(ex)) for ex in local}
  tadt = backend.torch_dtype(adt)
  bases = None
  if T > 1 or axis is None:
    tshape = tuple(T if d == ax else arr.shape[d] for d in range(nd))
    tot = torch.empty(tshape, dtype=tadt, device=ctx.device)
    be.fill(tot, backend.FILL_CONST, 0, 0, 0, (0,) * nd, tshape)
    for ex in local:
      o, n, i = axis_geom(ex.shape, ax)
      part = torch.empty((o, i), dtype=tadt, device=ctx.device)
      be.scan(data[ex], None, (o, n, i), totals=part)
      ul, shape = _bases_region(ex, ax, tids[ex.ul[ax]])
      be.copy_region(tot, ul, part.reshape(shape), (0,) * nd, shape)
    comm.all_reduce(tot, 'sum')
    bases = torch.empty(tshape, dtype=tadt, device=ctx.device)
    be.scan(tot, bases, (1, prod(tshape), 1) if axis is None else axis_geom(tshape, ax), exclusive=True)
  out_local = {}
  for ex in local:
    o, n, i = axis_geom(ex.shape, ax)
    carry = None
    if bases is not None:
      ul, shape = _bases_region(ex, ax, tids[ex.ul[ax]])
      carry = torch.empty((o, i), dtype=tadt, device=ctx.device)
      be.copy_region(carry.reshape(shape), (0,) * nd, bases, ul, shape)
    out = torch.empty(ex.shape, dtype=backend.torch_dtype(odt), device=ctx.device)
    be.scan(data[ex], out, (o, n, i), carry=carry)
    out_local[ex] = out
  return distarray.from_tiles(arr.shape, odt, arr.tiles, out_local)


# --------------------------------------------------------------- host path
def scan_array_host(arr, reduce_fn, scan_fn, axis):
  """The reference's steps with the caller's functions on host copies of the
  tiles: reduce_fn(tile, axis), scan_fn over the totals, tile[first] += base,
  scan_fn(tile, axis), upload (scan.py:24-64, :83-96)."""
  ctx = runtime.get()
  arr = with_tiles(arr)
  if arr.replicated:
    arr = distarray.from_numpy(arr.glom())
  nd = arr.ndim
  ax = nd - 1 if axis is None else axis
  tids = _axis_splits(arr, ax)
  T = len(tids)
  probe = np.zeros((1,) * nd, arr.dtype)
  tdt = np.asarray(reduce_fn(probe, axis=ax)).dtype
  odt = np.asarray(scan_fn(probe, axis=ax)).dtype
  tshape = tuple(T if d == ax else arr.shape[d] for d in range(nd))
  tot = np.zeros(tshape, tdt)
  tiles = {}
  for ex, w in arr.tiles.items():
    if not ctx.is_local(w):
      continue
    tile = transfer.download(backend.get().contiguous(arr.fetch(ex))).reshape(ex.shape)
    tiles[ex] = tile
    ul, shape = _bases_region(ex, ax, tids[ex.ul[ax]])
    tot[tuple(slice(u, u + s) for u, s in zip(ul, shape))] = np.asarray(reduce_fn(tile, axis=ax)).reshape(shape)
  if ctx.distributed:
    t = transfer.upload(tot, ctx.device)
    comm.all_reduce(t, 'sum')
    tot = transfer.download(t).reshape(tshape)
  if axis is None:
    flat = np.asarray(scan_fn(tot, axis=None)).reshape(-1)
    base = np.concatenate((np.zeros(1, flat.dtype), flat[:-1])).reshape(tshape)
  else:
    base = np.asarray(scan_fn(tot, axis=ax))
  out_local = {}
  for ex, tile in tiles.items():
    tile = tile.astype(odt)  # a copy: the mapper works on tile.copy()
    tid = tids[ex.ul[ax]]
    bid = tid if axis is None else tid - 1
    if bid >= 0:
      ul, shape = _bases_region(ex, ax, bid)
      first = tuple(slice(0, 1) if d == ax else slice(None) for d in range(nd))
      tile[first] += base[tuple(slice(u, u + s) for u, s in zip(ul, shape))].astype(odt)
    res = np.asarray(scan_fn(tile, axis=ax)).reshape(ex.shape)
    out_local[ex] = transfer.upload(np.ascontiguousarray(res), ctx.device)
  return distarray.from_tiles(arr.shape, odt, arr.tiles, out_local)

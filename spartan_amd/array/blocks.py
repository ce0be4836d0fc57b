"""Gather -- compute -- scatter over whole blocks: the routes every operation
takes that needs a line, a plane, a panel or a matrix in one place (sort,
topk, take / compress, stencil / maxpool, cholesky / solve_triangular, qr,
eigh, sparse dot).

``map_blocks(arr, axes, p, block)`` is the driver for one output array:

  1. ``arr`` replicated: every rank computes the whole and the result is a
     ``ReplicatedArray``; no exchange;
  2. every tile spans ``axes`` (``spans``): each tile is computed on its owner
     and the result is ``from_tiles`` over the same workers; no exchange;
  3. otherwise ``arr`` is cut along another axis ``p`` at its own tile cuts
     (``slabs``); each slab, complete along ``axes``, is brought to the owner
     of its first tile by ONE ``gather_regions`` (``gather_slabs``), computed
     there and delivered by ONE ``scatter_updates`` batch into a deferred
     target (``scatter_slabs``).  ``p = None`` is one slab: the whole array on
     the owner of its first tile, which must hold it.

An operation with a second output, or with a pass between the gather and the
compute, keeps its own loop over the same primitives.  ``whole`` is the other
recurring move: an array brought in full to every rank (or to some) by one
``gather_regions``.

The SPMD contract: every rank issues the same exchanges in the same order,
whether or not it owns tiles.  Everything here is decided from global metadata
(shapes, tile maps, worker ids), so callers keep it by calling these functions
on every rank.
"""
import numpy as np

from .. import backend, comm, runtime
from ..util import prod
from . import distarray
from . import extent as ext
from .tile import Tile


def with_tiles(arr):
  """``arr`` as an array with device tiles: a host value is distributed."""
  if isinstance(arr, distarray.LocalWrapper) and not isinstance(arr, distarray.ReplicatedArray):
    return distarray.from_numpy(np.asarray(arr.value))
  return arr


def axis_geom(shape, ax):
  """(outer, n, inner) of axis ``ax`` in a row-major block of ``shape``."""
  return prod(shape[:ax]), shape[ax], prod(shape[ax + 1:])


def spans(arr, axes):
  """Does every tile of ``arr`` cover each of ``axes`` in full?"""
  return all(e.ul[d] == 0 and e.lr[d] == arr.shape[d] for e in arr.tiles for d in axes)


def slabs(arr, p):
  """The array cut along axis p at every tile boundary along p:
  [(extent, worker of the first tile it overlaps)] in order.  ``p = None``:
  the whole array as one slab."""
  if p is None:
    full = ext.from_shape(arr.shape)
    return [(full, arr.tiles[min(arr.tiles, key=lambda e: e.ul)])]
  bounds = sorted({e.ul[p] for e in arr.tiles} | {e.lr[p] for e in arr.tiles})
  tiles = sorted(arr.tiles.items(), key=lambda kv: kv[0].ul)
  out = []
  for lo, hi in zip(bounds, bounds[1:]):
    ul = tuple(lo if d == p else 0 for d in range(arr.ndim))
    lr = tuple(hi if d == p else arr.shape[d] for d in range(arr.ndim))
    w = next(w for e, w in tiles if e.ul[p] <= lo < e.lr[p])
    out.append((ext.create(ul, lr, arr.shape), w))
  return out


def deferred(shape, dtype, tiles):
  """Unwritten array of ``shape`` with the tile map ``tiles`` ({extent: worker})."""
  ctx = runtime.get()
  tdt = backend.torch_dtype(dtype)
  local = {ex: Tile.deferred(ex.shape, tdt, ctx.device, ex) for ex, w in tiles.items() if ctx.is_local(w)}
  return distarray.DistArrayImpl(shape, dtype, dict(tiles), local)


def scatter_updates(target, updates):
  """Deliver every piece of ``updates`` -- [(order, target region, source rank,
  tensor on that rank or None)] -- to the owners of the target tiles it
  overlaps and merge them there in ``order``.  Collective."""
  import torch
  ctx = runtime.get()
  be = backend.get()
  tdt = backend.torch_dtype(target.dtype)
  sends, recvs, merges = [], [], []
  for order, tex, src, t in updates:
    if t is not None and t.dtype != tdt:  # pieces travel in the target dtype (the merge casts anyway)
      conv = torch.empty(t.shape, dtype=tdt, device=t.device)
      be.copy_region(conv, (0,) * t.dim(), t, (0,) * t.dim(), tuple(t.shape))
      t = conv
    if not tex.ndim:
      pairs = [(tile_ex, tex) for tile_ex in target.tiles]
    else:
      pairs = list(ext.find_overlapping(target.tiles, tex))
    for tile_ex, region in pairs:
      dst = ctx.owner(target.tiles[tile_ex])
      if src == ctx.rank:
        piece = t
        if tex.ndim and region != tex:
          rel = tuple(u - o for u, o in zip(region.ul, tex.ul))
          piece = torch.empty(region.shape, dtype=tdt, device=t.device)
          be.copy_region(piece, (0,) * region.ndim, t, rel, region.shape)
        if dst == ctx.rank:
          merges.append((order, tile_ex, region, piece))
        else:
          sends.append((piece, dst))
      elif dst == ctx.rank:
        buf = torch.empty(region.shape if region.ndim else (), dtype=tdt, device=ctx.device)
        recvs.append((buf, src))
        merges.append((order, tile_ex, region, buf))
  comm.exchange(sends, recvs)
  for order, tile_ex, region, piece in sorted(merges, key=lambda m: m[0]):
    tile = target.local[tile_ex]
    if not tile.written and region == tile_ex and tuple(region.lr) == tuple(tile_ex.lr) \
        and piece.is_contiguous() and tuple(piece.shape) == tuple(tile.shape):
      tile.data = piece  # first write of a whole tile: adopt the piece, no copy
      tile.written = [tile_ex]
      continue
    target.update(region, piece)


def whole(arr, ranks=None):
  """``arr`` as one contiguous device tensor on each rank of ``ranks``
  (default: every rank), None on a rank outside them.  A replicated array is
  at hand; any other takes ONE ``gather_regions`` with one request per rank of
  ``sorted(ranks)``.  Collective."""
  ctx = runtime.get()
  be = backend.get()
  if arr.replicated:
    return be.contiguous(arr.device_data())
  ranks = sorted(range(ctx.world_size) if ranks is None else ranks)
  full = ext.from_shape(arr.shape)
  got = distarray.gather_regions(arr, [(full, r) for r in ranks])
  return be.contiguous(got[ranks.index(ctx.rank)]) if ctx.rank in ranks else None


def gather_slabs(arr, p):
  """(``slabs(arr, p)``, {slab index: device block} of the slabs this rank
  computes): each slab brought to the owner of its first tile by one
  ``gather_regions``.  Collective."""
  ctx = runtime.get()
  sl = slabs(arr, p)
  return sl, distarray.gather_regions(arr, [(e, ctx.owner(w)) for e, w in sl])


def scatter_slabs(target, slabs, tensors, out_extent=None):
  """Deliver ``tensors`` ({slab index: result}, this rank's slabs) into
  ``target`` by one ``scatter_updates``: slab ``e`` lands on ``out_extent(e)``
  (default: ``e`` itself).  Collective."""
  ctx = runtime.get()
  scatter_updates(target, [((qi,), out_extent(e) if out_extent else e, ctx.owner(w), tensors.get(qi))
                           for qi, (e, w) in enumerate(slabs)])


def map_blocks(arr, axes, p, block, out_shape=None, out_extent=None, dtype=None, target=None):
  """``block(t, shape)`` -- the device block ``t`` of ``shape``, complete along
  ``axes``, to its result tensor -- over ``arr`` by the three routes of the
  module docstring; ``p`` is route 3's slab axis.  The result has ``out_shape``
  and ``dtype`` (default: arr's); the block at extent ``e`` lands on
  ``out_extent(e)`` (default: ``e``).  ``target(slabs)`` makes route 3's
  unwritten target; the default keeps arr's tile map (which needs the default
  ``out_shape``).  ``t`` comes as it is stored: ``block`` makes it contiguous
  if it has to be."""
  ctx = runtime.get()
  out_shape = tuple(arr.shape) if out_shape is None else tuple(out_shape)
  out_extent = out_extent or (lambda e: e)
  dtype = np.dtype(arr.dtype if dtype is None else dtype)
  if arr.replicated:  # one tile held in full by every rank
    return distarray.ReplicatedArray(block(arr.device_data(), tuple(arr.shape)))
  if spans(arr, axes):
    tiles = {out_extent(e): w for e, w in arr.tiles.items()}
    out_local = {out_extent(e): block(arr.fetch(e), e.shape) for e, w in arr.tiles.items() if ctx.is_local(w)}
    return distarray.from_tiles(out_shape, dtype, tiles, out_local)
  sl, got = gather_slabs(arr, p)
  out = target(sl) if target else deferred(out_shape, dtype, arr.tiles)
  scatter_slabs(out, sl, {qi: block(t, sl[qi][0].shape) for qi, t in got.items()}, out_extent)
  return out

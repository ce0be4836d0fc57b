"""``sort`` / ``argsort`` along an axis, ``partition`` / ``argpartition``
(the API of spartan/expr/sort.py).

The reference sorts with ``map2`` over tiles re-partitioned so that a tile
holds whole lines (sort.py:78-91, ``_sort_mapper`` = ``np.sort(tile, axis)``);
through ``change_partition_axis`` a 1-d array in several tiles is then sorted
tile by tile and a block partition raises.  That route is not restated: the
contract here is NumPy's result for ANY tile layout -- ``np.sort(a, axis)``
and ``np.argsort(a, axis, kind='stable')``, NaNs last, ``-0.0 == +0.0``.

A line has to be in one place to be sorted (``spx_sort``: LDS bitonic sort
for short lines, radix passes for long ones), so an integer axis takes the
three routes of ``array/blocks.py`` (``map_blocks``): a tile that spans the
whole axis is sorted on its owner, no exchange (the common case: row tiles
sorted along axis 1); otherwise the slabs are cut along ``p =
largest_dim_axis(shape, exclude_axes=[axis])`` and the target keeps the
input's tile layout.

A 1-d array in several tiles has no other axis to cut: it is gathered whole
to one owner, so it must fit in that GPU's memory next to the sort's
workspace (two key buffers, plus 32-bit positions for argsort).  The same
limit holds for ``sort(a, axis=None)``, the reference's meaning of which is
the flattened array sorted (a 1-d result of length ``size``): the flat array
is gathered to one owner, sorted as one long line and scattered into a fresh
1-d array.  (The reference's distributed sample sort, sort.py:93-108, is the
follow-up for arrays larger than one GPU's memory.)

Every rank issues the same exchanges whether or not it owns tiles.
``partition`` / ``argpartition`` return the full sort / argsort, which
satisfies NumPy's partition contract; ``kth`` is range-checked only.
"""
import numpy as np

from .. import backend
from ..array import distarray
from ..array import extent as ext
from ..array.blocks import axis_geom, gather_slabs, map_blocks, scatter_slabs, with_tiles
from ..util import prod
from .base import Expr, as_array


class SortExpr(Expr):
  _members = ('array',)

  def compute_shape(self):
    if self.axis is None:
      return (prod(self.array.shape),)
    return self.array.shape

  def compute_dtype(self):
    return np.dtype(np.int64) if self.want_idx else np.dtype(self.array.dtype)

  def pretty_str(self):
    return '%s[%d](%s, axis=%s)' % ('Argsort' if self.want_idx else 'Sort', self.expr_id, self.array, self.axis)

  def _evaluate(self, deps):
    return sort_array(distarray.as_array(deps['array']), self.axis, self.want_idx)


def _make(array, axis, want_idx, name):
  array = as_array(array)
  nd = len(array.shape)
  if nd == 0:
    raise ValueError('%s: a 0-d array has no axis to sort' % name)
  if axis is not None:
    if not isinstance(axis, (int, np.integer)) or not -nd <= axis < nd:
      raise ValueError('%s: axis %r is out of range for a %d-d array' % (name, axis, nd))
    axis = int(axis) % nd
  e = SortExpr(array=array)
  e.axis = axis
  e.want_idx = bool(want_idx)
  return e


def sort(array, axis=-1):
  """``np.sort(array, axis)``, lazily; ``axis=None`` sorts the flattened
  array (a 1-d result).  A 1-d array, and any array with ``axis=None``, is
  gathered whole to one GPU: that GPU's memory is the limit."""
  return _make(array, axis, False, 'sort')


def argsort(array, axis=-1):
  """``np.argsort(array, axis, kind='stable')`` (int64), lazily."""
  assert axis is not None, "Spartan doesn't support argsort when axis == None"
  return _make(array, axis, True, 'argsort')


def _check_kth(array, kth, axis, name):
  assert axis is not None, "Spartan doesn't support %s when axis == None" % name
  e = _make(array, axis, name == 'argpartition', name)
  n = e.array.shape[e.axis]
  for k in np.atleast_1d(np.asarray(kth)).tolist():
    if not isinstance(k, int) or not -n <= k < n:
      raise ValueError('%s: kth %r is out of bounds for an axis of length %d' % (name, k, n))
  return e


def partition(array, kth, axis=-1):
  """``np.partition``'s contract by the full sort (no selection kernel)."""
  return _check_kth(array, kth, axis, 'partition')


def argpartition(array, kth, axis=-1):
  """``np.argpartition``'s contract by the full stable argsort."""
  return _check_kth(array, kth, axis, 'argpartition')


# ------------------------------------------------------------- evaluation
def _sort_block(t, shape, ax, want_idx):
  """Sorted values / argsort of the device block ``t`` of ``shape`` along ax."""
  import torch
  be = backend.get()
  src = be.contiguous(t)
  odt = np.int64 if want_idx else backend.np_dtype(src.dtype)
  out = torch.empty(tuple(shape), dtype=backend.torch_dtype(odt), device=src.device)
  be.sort(src, None if want_idx else out, out if want_idx else None, axis_geom(shape, ax))
  return out


def sort_array(arr, axis, want_idx):
  be = backend.get()
  arr = with_tiles(arr)
  if arr.ndim == 0:
    raise ValueError('sort: a 0-d array has no axis to sort')
  odt = np.dtype(np.int64) if want_idx else np.dtype(arr.dtype)
  backend.spx_dtype(arr.dtype)
  size = prod(arr.shape)
  if size == 0 and not arr.replicated:
    return distarray.create((0,) if axis is None else arr.shape, odt)
  if axis is not None:
    p = ext.largest_dim_axis(arr.shape, exclude_axes=[axis]) if arr.ndim > 1 else None
    return map_blocks(arr, (axis,), p, lambda t, shape: _sort_block(t, shape, axis, want_idx), dtype=odt)
  if arr.replicated:  # one tile held in full by every rank
    return distarray.ReplicatedArray(_sort_block(arr.device_data(), (size,), 0, want_idx))
  slabs, got = gather_slabs(arr, None)
  target = distarray.create((size,), odt)
  flat = {qi: _sort_block(be.contiguous(t).reshape(-1), (size,), 0, False) for qi, t in got.items()}
  scatter_slabs(target, slabs, flat, lambda e: ext.from_shape((size,)))
  return target

"""``topk`` / ``argtopk`` along an axis: the first ``k`` of each line's stable
order, by selection (``spx_topk``) instead of the full sort.

The reference has no selection: its nearest-neighbour search sorts the whole
distance matrix and keeps ``[:, :k]`` (spartan/examples/sklearn/neighbors/
unsupervised.py).  The contract here, for a line ``x`` of length n and
``1 <= k <= n``:

  * ``largest=False``: positions ``np.argsort(x, kind='stable')[:k]`` -- the
    order of ``sort`` / ``argsort`` (NaNs last, ``-0.0 == +0.0``, ties keep
    input order);
  * ``largest=True``: descending by value, equal keys lower position first,
    NaNs still last -- ``np.argsort(-x, kind='stable')[:k]`` for floats,
    ``np.argsort(~x, kind='stable')[:k]`` for integers and bool.

The result has the input's shape with ``axis`` replaced by ``k``.  A line has
to be in one place to be selected from, so the routes are ``sort_array``'s,
the three of ``array/blocks.py``; route 3 delivers into a fresh array of the
result's shape in the default layout.  Every rank issues the same exchanges.

``k`` above ``backend.TOPK_K_MAX`` (the candidates of a line are ordered by
one LDS sort): ``largest=False`` goes through ``sort`` / ``argsort`` and a
slice; ``largest=True`` raises ``NotImplementedError``.
"""
import numpy as np

from .. import backend
from ..array import distarray
from ..array import extent as ext
from ..array.blocks import axis_geom, map_blocks, with_tiles
from ..util import prod
from .base import Expr, as_array
from .sort import argsort, sort


class TopkExpr(Expr):
  _members = ('array',)

  def compute_shape(self):
    shape = self.array.shape
    return shape[:self.axis] + (self.k,) + shape[self.axis + 1:]

  def compute_dtype(self):
    return np.dtype(np.int64) if self.want_idx else np.dtype(self.array.dtype)

  def pretty_str(self):
    return '%s[%d](%s, k=%d, axis=%d, largest=%s)' % ('Argtopk' if self.want_idx else 'Topk', self.expr_id,
                                                      self.array, self.k, self.axis, self.largest)

  def _evaluate(self, deps):
    return topk_array(distarray.as_array(deps['array']), self.k, self.axis, self.largest, self.want_idx)


def _make(array, k, axis, largest, want_idx, name):
  array = as_array(array)
  nd = len(array.shape)
  if nd == 0:
    raise ValueError('%s: a 0-d array has no axis to select along' % name)
  assert axis is not None, "Spartan doesn't support %s when axis == None" % name
  if not isinstance(axis, (int, np.integer)) or not -nd <= axis < nd:
    raise ValueError('%s: axis %r is out of range for a %d-d array' % (name, axis, nd))
  axis = int(axis) % nd
  n = array.shape[axis]
  if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= n:
    raise ValueError('%s: k %r is outside [1, %d]' % (name, k, n))
  k = int(k)
  if k > backend.TOPK_K_MAX:
    if largest:
      raise NotImplementedError('%s: largest=True supports k up to TOPK_K_MAX = %d, got %d'
                                % (name, backend.TOPK_K_MAX, k))
    full = argsort(array, axis) if want_idx else sort(array, axis)
    return full[tuple(slice(0, k) if d == axis else slice(None) for d in range(nd))]
  e = TopkExpr(array=array)
  e.axis = axis
  e.k = k
  e.largest = bool(largest)
  e.want_idx = bool(want_idx)
  return e


def topk(array, k, axis=-1, largest=False):
  """The ``k`` smallest (``largest``: largest) values along ``axis`` in
  order, lazily; the result's shape is the input's with ``axis`` -> ``k``."""
  return _make(array, k, axis, largest, False, 'topk')


def argtopk(array, k, axis=-1, largest=False):
  """The int64 positions along ``axis`` of ``topk``'s values, lazily."""
  return _make(array, k, axis, largest, True, 'argtopk')


# ------------------------------------------------------------- evaluation
def _out_shape(shape, ax, k):
  return tuple(shape[:ax]) + (k,) + tuple(shape[ax + 1:])


def _topk_block(t, shape, ax, k, largest, want_idx):
  """Selected values / positions of the device block ``t`` of ``shape``."""
  import torch
  be = backend.get()
  src = be.contiguous(t)
  odt = np.int64 if want_idx else backend.np_dtype(src.dtype)
  out = torch.empty(_out_shape(shape, ax, k), dtype=backend.torch_dtype(odt), device=src.device)
  be.topk(src, None, None if want_idx else out, out if want_idx else None, axis_geom(shape, ax), k, largest)
  return out


def _out_extent(e, ax, k, out_shape):
  ul = tuple(0 if d == ax else e.ul[d] for d in range(e.ndim))
  lr = tuple(k if d == ax else e.lr[d] for d in range(e.ndim))
  return ext.create(ul, lr, out_shape)


def topk_array(arr, k, axis, largest, want_idx):
  arr = with_tiles(arr)
  if arr.ndim == 0:
    raise ValueError('topk: a 0-d array has no axis to select along')
  odt = np.dtype(np.int64) if want_idx else np.dtype(arr.dtype)
  backend.spx_dtype(arr.dtype)
  out_shape = _out_shape(arr.shape, axis, k)
  if prod(out_shape) == 0 and not arr.replicated:
    return distarray.create(out_shape, odt)
  p = ext.largest_dim_axis(arr.shape, exclude_axes=[axis]) if arr.ndim > 1 else None
  return map_blocks(arr, (axis,), p, lambda t, shape: _topk_block(t, shape, axis, k, largest, want_idx),
                    out_shape=out_shape, out_extent=lambda e: _out_extent(e, axis, k, out_shape), dtype=odt,
                    target=lambda slabs: distarray.create(out_shape, odt))

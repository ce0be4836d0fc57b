"""``stencil`` (2-d convolution) and ``maxpool`` -- the convnet pair of
spartan/expr/stencil.py, with the reference's signatures.

``stencil(images, filters, stride=1)``: images (N, C, W, H), filters (F, C,
fw, fh), result (N, F, W, H) in the images' dtype (float32 / float64),

  out[n, f, x, y] = sum over c < C, i < fw, j < fh with x + i < W and y + j < H
                    of images[n, c, x + i, y + j] * filters[f, c, i, j]

-- the reference's ``_convolve`` (stencil.py:27-43): cross-correlation anchored
at the top-left, taps past the bottom / right edge dropped.

  * ``stride`` is accepted and ignored, as in the reference: its ``stencil``
    never reads the argument (its test_convnet passes 2 and goes on with
    full-size outputs).  A wart kept on purpose.
  * The result is that formula on the WHOLE array for any tile layout.  The
    reference convolves each tile on its own and clips at tile borders, so a
    spatially tiled input loses the taps that cross a tile edge; that is not
    restated (the decision taken for sort).
  * Evaluation is lazy like every other node; the reference forces ``images``
    inside ``stencil``.  Forcing the node gives the same value.

``maxpool(images, pool_size=2, stride=2)``: result (N, C, ceil(W / stride),
ceil(H / stride)) in the images' dtype (the five dtypes, bool as bytes),

  out[n, c, p, q] = max over i, j < pool_size with p stride + i < W and
                    q stride + j < H of images[n, c, p stride + i, q stride + j]

-- the loop the reference's ``_maxpool`` has in its commented-out lines
(stencil.py:58-67).  Its live body is a stub left by a compiler bug and
returns a constant array: the intent is restated, not the stub.  Every window
holds its first element, so there is no fill value (no -1e12); NaN propagates
as in ``np.maximum``.

Tiles.  Both need whole (W, H) planes -- stencil all C of them -- in one
place, by the three routes of ``array/blocks.py`` (``map_blocks``):

  * every tile spans (C, W, H) (images dealt along axis 0, the benchmark's
    layout): each tile is convolved / pooled on its owner, the output keeps
    the input's cuts along axis 0 and no array data moves;
  * any other layout (the reference's tests tile the two spatial axes): slabs
    along axis 0, delivered into a target tiled along axis 0 at the same
    cuts.  Limit: one slab and its output must fit on one GPU (a halo
    exchange between spatial tiles is the follow-up);
  * a replicated / host input gives a replicated result.

``filters`` (an expression, an array or a NumPy array) is brought whole to
every rank, as the reference's ``filters.glom()`` does.  An ``images`` array
without elements gives a host array of the result's shape.
"""
import numpy as np

from .. import backend
from ..array import distarray
from ..array import extent as ext
from ..array.blocks import deferred, map_blocks, whole
from ..util import prod
from .base import Expr, as_array

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


class StencilExpr(Expr):
  _members = ('images', 'filters')

  def compute_shape(self):
    n, _, w, h = self.images.shape
    return (n, self.filters.shape[0], w, h)

  def compute_dtype(self):
    return np.dtype(self.images.dtype)

  def pretty_str(self):
    return 'Stencil[%d](%s, %s)' % (self.expr_id, self.images, self.filters)

  def _evaluate(self, deps):
    return stencil_array(distarray.as_array(deps['images']), distarray.as_array(deps['filters']))


class MaxpoolExpr(Expr):
  _members = ('images',)

  def compute_shape(self):
    n, c, w, h = self.images.shape
    return (n, c, -(-w // self.stride), -(-h // self.stride))

  def compute_dtype(self):
    return np.dtype(self.images.dtype)

  def pretty_str(self):
    return 'Maxpool[%d](%s, pool_size=%d, stride=%d)' % (self.expr_id, self.images, self.pool_size, self.stride)

  def _evaluate(self, deps):
    return maxpool_array(distarray.as_array(deps['images']), self.pool_size, self.stride)


def stencil(images, filters, stride=1):
  """Convolve ``images`` (N, C, W, H) with ``filters`` (F, C, fw, fh), lazily:
  the module's formula on the whole array.  ``stride`` is accepted and
  ignored, as in the reference."""
  images, filters = as_array(images), as_array(filters)
  idt, fdt = np.dtype(images.dtype), np.dtype(filters.dtype)
  for what, dt in (('images', idt), ('filters', fdt)):
    if dt not in _FLOATS:
      raise TypeError('stencil: %s of dtype %s have no gfx950 path (float32 / float64)' % (what, dt))
  if idt != fdt:
    raise TypeError('stencil: images are %s and filters %s: one dtype is needed' % (idt, fdt))
  if len(images.shape) != 4 or len(filters.shape) != 4:
    raise ValueError('stencil: images (N, C, W, H) and filters (F, C, fw, fh) must be 4-d, not %d-d and %d-d'
                     % (len(images.shape), len(filters.shape)))
  if images.shape[1] != filters.shape[1]:
    raise ValueError('stencil: images have %d channels, filters %d' % (images.shape[1], filters.shape[1]))
  if prod(filters.shape) == 0:
    raise ValueError('stencil: filters of shape %s have no elements' % (tuple(filters.shape),))
  return StencilExpr(images=images, filters=filters)


def _positive_int(v, name):
  if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
    raise ValueError('maxpool: %s must be an integer of at least 1, not %r' % (name, v))
  return int(v)


def maxpool(images, pool_size=2, stride=2):
  """The maximum over ``pool_size`` x ``pool_size`` windows of the last two
  axes of ``images`` (N, C, W, H), every ``stride`` elements, lazily; windows
  are clipped at the bottom / right edge."""
  images = as_array(images)
  pool_size, stride = _positive_int(pool_size, 'pool_size'), _positive_int(stride, 'stride')
  backend.spx_dtype(images.dtype)
  if len(images.shape) != 4:
    raise ValueError('maxpool: images (N, C, W, H) must be 4-d, not %d-d' % len(images.shape))
  e = MaxpoolExpr(images=images)
  e.pool_size = pool_size
  e.stride = stride
  return e


# ------------------------------------------------------------- evaluation
def _planes(arr, oshape, block):
  """``block(t)`` -- (n, C, W, H) contiguous device block -> (n,) + oshape[1:]
  -- over ``arr`` along axis 0, by the three routes of the module docstring."""
  be = backend.get()
  oshape = tuple(int(s) for s in oshape)
  if prod(arr.shape) == 0 or prod(oshape) == 0:
    return distarray.LocalWrapper(np.empty(oshape, np.dtype(arr.dtype)))
  out_ex = lambda e: ext.create((e.ul[0], 0, 0, 0), (e.lr[0],) + oshape[1:], oshape)
  return map_blocks(arr, (1, 2, 3), 0, lambda t, shape: block(be.contiguous(t)), out_shape=oshape, out_extent=out_ex,
                    target=lambda slabs: deferred(oshape, arr.dtype, {out_ex(e): w for e, w in slabs}))


def stencil_array(images, filters):
  import torch
  be = backend.get()
  n, c, w, h = images.shape
  f = filters.shape[0]
  flt = whole(filters)  # a collective: before any early return that depends on the images' layout only

  def block(t):
    out = torch.empty((t.shape[0], f, w, h), dtype=t.dtype, device=t.device)
    be.stencil(t, flt, out)
    return out
  return _planes(images, (n, f, w, h), block)


def maxpool_array(images, pool_size, stride):
  import torch
  be = backend.get()
  n, c, w, h = images.shape
  p, q = -(-w // stride), -(-h // stride)

  def block(t):
    out = torch.empty((t.shape[0], c, p, q), dtype=t.dtype, device=t.device)
    be.maxpool(t, out, pool_size, stride)
    return out
  return _planes(images, (n, c, p, q), block)

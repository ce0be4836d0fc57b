"""Shared by tests/test_stencil.py and tests/test_stencil_gpu.py: the NumPy
contract of ``stencil`` / ``maxpool`` (spartan_amd/expr/stencil.py), the data
makers of both files and the CPU test double's ``stencil`` / ``maxpool``
(HipBackend's signatures and argument contracts)."""
import math

import numpy as np

from spartan_amd import backend as B
from fake_backend import FakeBackend, _np, _put


def _taps(images, filters):
  """float64 sum over the fw * fh taps of shifted slices, one einsum per tap."""
  n, c, w, h = images.shape
  f, fc, fw, fh = filters.shape
  assert c == fc, (images.shape, filters.shape)
  out = np.zeros((n, f, w, h), np.float64)
  for i in range(min(fw, w)):
    for j in range(min(fh, h)):
      out[:, :, :w - i, :h - j] += np.einsum('ncxy,fc->nfxy', images[:, :, i:, j:], filters[:, :, i, j])
  return out


def stencil_ref(images, filters):
  """out[n, f, x, y] = sum over c, i, j with x + i < W, y + j < H of
  images[n, c, x + i, y + j] * filters[f, c, i, j], accumulated in float64."""
  return _taps(np.asarray(images, np.float64), np.asarray(filters, np.float64))


def stencil_mag(images, filters):
  """The same sum over absolute values: the scale of a tolerance."""
  return _taps(np.abs(np.asarray(images, np.float64)), np.abs(np.asarray(filters, np.float64)))


def maxpool_ref(a, pool, stride):
  """out[n, c, p, q] = max over i, j < pool with p stride + i < W, q stride + j
  < H of a[n, c, p stride + i, q stride + j], by window slices; NaN propagates
  (np.maximum).  The window's first element always exists."""
  a = np.asarray(a)
  n, c, w, h = a.shape
  out = a[:, :, ::stride, ::stride].copy()
  for i in range(min(pool, w)):
    for j in range(min(pool, h)):
      v = a[:, :, i::stride, j::stride]
      sub = out[:, :, :v.shape[2], :v.shape[3]]
      np.maximum(sub, v, out=sub)
  assert out.shape == (n, c, -(-w // stride), -(-h // stride))
  return out


def int_data(shape, dtype, seed):
  """Integer-valued data in [-4, 4]: sums of products stay exact in fp32."""
  return np.random.RandomState(seed).randint(-4, 5, shape).astype(dtype)


def normal_data(shape, dtype, seed):
  return np.random.RandomState(seed).standard_normal(shape).astype(dtype)


def pool_data(shape, dtype, seed):
  """Values of any of the five dtypes with repeats (ties inside a window)."""
  r = np.random.RandomState(seed)
  dt = np.dtype(dtype)
  if dt == np.bool_:
    return r.randint(0, 2, shape) > 0
  if dt.kind == 'i':
    big = int(np.iinfo(dt).max // 2)
    return (r.randint(-9, 10, shape).astype(dt) * dt.type(big // 9))
  return (r.randint(-9, 10, shape) * 0.25).astype(dt)


class StencilFakeBackend(FakeBackend):
  """FakeBackend + NumPy ``stencil`` / ``maxpool``."""

  def stencil(self, images, filters, out):
    dt = B.np_dtype(images.dtype)
    assert dt in (np.float32, np.float64) and filters.dtype == images.dtype and out.dtype == images.dtype
    assert images.dim() == 4 and filters.dim() == 4 and images.shape[1] == filters.shape[1]
    assert images.is_contiguous() and filters.is_contiguous() and out.is_contiguous()
    assert tuple(out.shape) == (images.shape[0], filters.shape[0], images.shape[2], images.shape[3])
    assert min(filters.shape) > 0 and min(images.shape[1:]) > 0
    self.calls.append('stencil')
    if images.shape[0] == 0:
      return
    _put(out, stencil_ref(_np(images), _np(filters)).astype(dt))

  def maxpool(self, src, out, pool_size, stride):
    assert pool_size >= 1 and stride >= 1
    assert src.dim() == 4 and out.dtype == src.dtype and src.is_contiguous() and out.is_contiguous()
    n, c, w, h = src.shape
    assert tuple(out.shape) == (n, c, -(-w // stride), -(-h // stride))
    self.calls.append('maxpool')
    if n == 0:
      return
    _put(out, maxpool_ref(_np(src), pool_size, stride))


ONE_TILE = (10000, 10000, 10000, 10000)


def _divup(a, b):
  return int(math.ceil(float(a) / float(b)))


def layouts(shape):
  """Tile hints of an (N, C, W, H) array: default, cuts along axis 0, along
  each spatial axis, 2 x 2 spatial blocks, cuts along C."""
  n, c, w, h = shape
  return [None,
          (_divup(n, 3), c, w, h),
          (n, c, _divup(w, 2), h),
          (n, c, w, _divup(h, 3)),
          (n, c, _divup(w, 2), _divup(h, 2)),
          (n, _divup(c, 2), w, h)]


# ------------------------------------------------- the reference's drivers
def driver_test_stencil(expr, stencil, num_workers):
  """tests/test_stencil.py::test_stencil of the reference, at its sizes."""
  img = int(8 * math.sqrt(num_workers))
  filt, n, f = 8, 8, 32
  tile = _divup(img, math.sqrt(num_workers))
  images = expr.ones((n, 3, img, img), dtype=np.float64, tile_hint=(n, 3, tile, tile))
  filters = expr.ones((f, 3, filt, filt), dtype=np.float64, tile_hint=ONE_TILE)
  return stencil.stencil(images, filters, 1), np.ones((n, 3, img, img)), np.ones((f, 3, filt, filt))


def driver_test_convnet(expr, stencil, num_workers, dtype=np.float64, data=None):
  """tests/test_convnet.py::test_convnet: three conv + pool layers, stride=2
  passed through to stencil (and ignored).  ``data(shape, seed)`` replaces the
  reference's ones."""
  colors, size, fs, n_imgs, n_filt = 3, 16, (5, 5), 1, 1
  hint = _divup(64, math.sqrt(num_workers))
  mk = (lambda shape, seed: np.ones(shape, dtype)) if data is None else data
  a = mk((n_imgs, colors, size, size), 1)
  ws = [mk((n_filt, colors) + fs, 2), mk((n_filt, n_filt) + fs, 3), mk((n_filt, n_filt) + fs, 4)]
  x = expr.eager(expr.from_numpy(a, tile_hint=(n_imgs, colors, hint, hint)))
  for w in ws:
    wx = expr.eager(expr.from_numpy(w, tile_hint=ONE_TILE))
    x = stencil.maxpool(stencil.stencil(x, wx, 2))
  return x, a, ws


def convnet_ref(a, ws):
  """The three conv + pool(2, 2) layers on host arrays, each layer in a's dtype."""
  for w in ws:
    a = maxpool_ref(stencil_ref(a, w).astype(a.dtype), 2, 2)
  return a


def driver_benchmark(expr, stencil, num_workers, minibatch=8, size=16, n_filt=4, dtype=np.float64, data=None):
  """tests/benchmark_convnet.py::benchmark_convnet at a small size: images
  dealt along axis 0, 4 x 4 filters, three conv + pool layers."""
  colors, fs = 3, (4, 4)
  tile_hint = (_divup(minibatch, num_workers), colors, size, size)
  mk = (lambda shape, seed: np.ones(shape, dtype)) if data is None else data
  a = mk((minibatch, colors, size, size), 5)
  ws = [mk((n_filt, colors) + fs, 6), mk((n_filt, n_filt) + fs, 7), mk((n_filt, n_filt) + fs, 8)]
  x = expr.eager(expr.from_numpy(a, tile_hint=tile_hint))
  for w in ws:
    wx = expr.eager(expr.from_numpy(w, tile_hint=ONE_TILE))
    x = stencil.maxpool(stencil.stencil(x, wx, 2))
  return x, a, ws

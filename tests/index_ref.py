"""Shared by tests/test_index.py and tests/test_index_gpu.py: the NumPy
``take`` / ``compact_count`` / ``compact`` the CPU test double gets
(HipBackend's signatures and contracts on the (outer, n, inner) view) and the
mask / index generators of both files."""
import numpy as np
import torch

from spartan_amd import backend as B
from fake_backend import _np, _put
from sort_ref import SortFakeBackend


class IndexFakeBackend(SortFakeBackend):
  """FakeBackend + NumPy ``sort`` / ``take`` / ``compact_count`` / ``compact``."""

  def take(self, src, idx, out, geom, lo, n_total, out_strides=None):
    o, nl, i = (int(v) for v in geom)
    assert src.is_contiguous() and src.numel() == o * nl * i
    assert idx.dim() == 1 and idx.is_contiguous() and B.np_dtype(idx.dtype) in (np.int32, np.int64)
    assert out.dtype == src.dtype and out.is_contiguous()
    assert 0 <= lo and lo + nl <= n_total
    self.calls.append('take')
    m = idx.numel()
    if o == 0 or m == 0 or i == 0:
      return
    oos, ors = (m * i, i) if out_strides is None else (int(v) for v in out_strides)
    assert ors >= i and (o - 1) * oos + (m - 1) * ors + i <= out.numel()
    x = _np(src).reshape(o, nl, i)
    r = _np(idx).astype(np.int64)
    r = np.where(r < 0, r + n_total, r)
    bad = (r < 0) | (r >= n_total)
    flat = _np(out).reshape(-1).copy()
    for j in np.nonzero(~bad & (r >= lo) & (r < lo + nl))[0]:
      for oo in range(o):
        p = oo * oos + j * ors
        flat[p:p + i] = x[oo, r[j] - lo]
    _put(out, flat.reshape(out.shape))
    if bad.any():
      raise IndexError('take: an index is out of bounds for an axis of length %d' % n_total)

  def compact_count(self, mask):
    assert mask.is_contiguous() and mask.element_size() == 1
    self.calls.append('compact_count')
    if mask.numel() == 0:
      return 0, None
    return int(np.count_nonzero(_np(mask))), torch.as_tensor(_np(mask).reshape(-1).copy())

  def compact(self, src, mask, out, geom, workspace):
    o, n, i = (int(v) for v in geom)
    assert src.is_contiguous() and src.numel() == o * n * i
    assert mask.is_contiguous() and mask.element_size() == 1 and mask.numel() == n
    assert out.dtype == src.dtype and out.is_contiguous()
    self.calls.append('compact')
    if o * i == 0 or n == 0 or out.numel() == 0:
      return
    sel = _np(mask).reshape(-1) != 0
    assert workspace is not None and np.array_equal(_np(workspace) != 0, sel)  # the workspace of this very mask
    assert out.numel() == o * int(sel.sum()) * i
    _put(out, _np(src).reshape(o, n, i)[:, sel, :])


def bits(a):
  """The bytes of ``a`` (comparisons by bit pattern)."""
  return np.ascontiguousarray(a).view(np.uint8)


MASK_KINDS = ['none', 'all', 'first', 'last', 'alternating', 'runs', 'half', 'sparse', 'tiles']


def mask_data(n, kind, seed, tile=4096):
  """n mask BYTES (uint8; nonzero selects, and not only 1).  kind: 'none',
  'all', 'first' / 'last' (one element), 'alternating', 'runs' (random runs of
  up to 100), 'half' / 'sparse' (random at densities 1/2 and 1/64), 'tiles'
  (whole tiles of ``tile`` bytes alternately full and empty)."""
  r = np.random.RandomState(seed)
  m = np.zeros(n, np.uint8)
  if kind == 'all':
    m[:] = 1
  elif kind == 'first':
    m[:1] = 1
  elif kind == 'last':
    m[-1:] = 1
  elif kind == 'alternating':
    m[::2] = 1
  elif kind == 'runs':
    pos, on = 0, bool(seed & 1)
    while pos < n:
      ln = int(r.randint(1, 101))
      m[pos:pos + ln] = on
      pos += ln
      on = not on
  elif kind == 'half':
    m[:] = r.random_sample(n) < 0.5
  elif kind == 'sparse':
    m[:] = r.random_sample(n) < 1.0 / 64
  elif kind == 'tiles':
    m[:] = ((np.arange(n) // tile) % 2 == 0)
  else:
    assert kind == 'none', kind
  # any nonzero byte selects: vary the selecting byte's value
  return (m * r.randint(1, 256, n)).astype(np.uint8)


INDEX_KINDS = ['identity', 'reversed', 'equal', 'random', 'negative']


def index_data(n, m, kind, seed, dtype=np.int64):
  """m indices into an axis of length n.  kind: 'identity' (0..m-1 mod n),
  'reversed', 'equal' (one value), 'random' (with duplicates, both signs),
  'negative' (all negative)."""
  r = np.random.RandomState(seed)
  if kind == 'identity':
    x = np.arange(m) % n
  elif kind == 'reversed':
    x = (n - 1 - np.arange(m)) % n
  elif kind == 'equal':
    x = np.full(m, int(r.randint(0, n)))
  elif kind == 'negative':
    x = r.randint(-n, 0, m)
  else:
    assert kind == 'random', kind
    x = r.randint(-n, n, m)
  return x.astype(dtype)


def values(shape, dtype, seed):
  """Test values with the bit patterns that must survive: -0.0, NaNs with
  payloads, all 32 / 64 bits of the integers."""
  r = np.random.RandomState(seed)
  dt = np.dtype(dtype)
  n = int(np.prod(shape))
  if dt == np.bool_:
    return (r.randint(0, 2, n) > 0).reshape(shape)
  if dt.kind == 'i':
    b = r.randint(0, 256, n * dt.itemsize).astype(np.uint8)
    return b.view(dt).reshape(shape)
  x = (r.randint(-4, 5, n) * 0.5).astype(dt)
  ut = np.uint32 if dt.itemsize == 4 else np.uint64
  nan = (np.array([0x7FC00000], np.uint32) if dt.itemsize == 4 else np.array([0x7FF8000000000000], np.uint64))
  pick = r.random_sample(n)
  xb = x.view(ut)
  sel = pick > 0.9
  xb[sel] = nan[0] | r.randint(1, 1 << 16, int(sel.sum())).astype(ut)  # NaN payloads
  x[pick < 0.1] = -0.0
  return x.reshape(shape)

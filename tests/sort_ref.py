"""Shared by tests/test_sort.py and tests/test_sort_gpu.py: the NumPy ``sort``
the CPU test double gets (HipBackend.sort's signature and order contract:
np.sort / np.argsort(kind='stable') on the (outer, n, inner) view) and the
data generators of both files."""
import numpy as np

from spartan_amd import backend as B
from fake_backend import FakeBackend, _np, _put


class SortFakeBackend(FakeBackend):
  """FakeBackend + a NumPy ``sort``."""

  def sort(self, src, out_vals, out_idx, axis_geom):
    o, n, i = (int(v) for v in axis_geom)
    assert src.is_contiguous() and src.numel() == o * n * i
    assert out_vals is not None or out_idx is not None
    x = _np(src).reshape(o, n, i)
    if out_vals is not None:
      assert out_vals.dtype == src.dtype and out_vals.numel() == src.numel() and out_vals.is_contiguous()
      _put(out_vals, np.sort(x, axis=1, kind='stable'))
    if out_idx is not None:
      assert B.np_dtype(out_idx.dtype) == np.int64 and out_idx.numel() == src.numel() and out_idx.is_contiguous()
      _put(out_idx, np.argsort(x, axis=1, kind='stable').astype(np.int64))
    self.calls.append('sort')


def kat_ints(shape, seed):
  """The reference KAT's values: int(randn * 100)."""
  r = np.random.RandomState(seed)
  return (r.randn(*shape) * 100).astype(np.int64)


FLOAT_SPECIALS = {
    np.dtype(np.float32): [-np.inf, np.inf, -0.0, 0.0, 1e-45, -1e-45, 1e-40, np.finfo(np.float32).max,
                           -np.finfo(np.float32).max, np.finfo(np.float32).tiny],
    np.dtype(np.float64): [-np.inf, np.inf, -0.0, 0.0, 5e-324, -5e-324, 1e-310, np.finfo(np.float64).max,
                           -np.finfo(np.float64).max, np.finfo(np.float64).tiny],
}


def _nan(dt, negative, payload):
  """A NaN of ``dt`` with the given sign and a payload in the low bits."""
  if dt == np.float32:
    bits = np.uint32(0x7FC00000 | (payload & 0xFFFF) | (0x80000000 if negative else 0))
    return np.array([bits], np.uint32).view(np.float32)[0]
  bits = np.uint64(0x7FF8000000000000 | (payload & 0xFFFF) | (0x8000000000000000 if negative else 0))
  return np.array([bits], np.uint64).view(np.float64)[0]


def key_bits(dt):
  return 8 if np.dtype(dt) == np.bool_ else 8 * np.dtype(dt).itemsize


def sort_data(shape, dtype, kind, seed, digit=0):
  """(outer, n, inner) test data.  kind:
    'uniform'  the full range of the type (int32: all 32 bits, int64: +-2^62,
               floats: random bit patterns of finite values);
    'dup7'     keys from a range of 7 values (stability);
    'equal'    all keys equal;
    'asc' / 'desc'  sorted input along n;
    'digit'    keys that differ in radix digit ``digit`` (8 bits) only;
    'extremes' ints: INT_MIN / -1 / 0 / INT_MAX; floats: +-inf, +-0.0,
               denormals, the largest values, and NaNs of both signs with
               payloads at about 5 %, among small random values."""
  r = np.random.RandomState(seed)
  dt = np.dtype(dtype)
  o, n, i = shape
  if dt == np.bool_:
    if kind == 'equal':
      return np.ones(shape, np.bool_)
    x = r.randint(0, 2, shape) > 0
    if kind in ('asc', 'desc'):
      x = np.sort(x, axis=1)
      return x[:, ::-1, :].copy() if kind == 'desc' else x
    return x
  ut = {4: np.uint32, 8: np.uint64}[dt.itemsize]
  if kind == 'uniform':
    if dt == np.int32:
      return r.randint(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
    if dt == np.int64:
      return r.randint(-2 ** 62, 2 ** 62, shape, dtype=np.int64)
    bits = r.randint(0, 2 ** 32, shape, dtype=np.int64).astype(np.uint64)
    if dt.itemsize == 8:
      bits = (bits << np.uint64(32)) | r.randint(0, 2 ** 32, shape, dtype=np.int64).astype(np.uint64)
    x = bits.astype(ut).view(dt)
    return np.where(np.isfinite(x), x, dt.type(1.5))
  if kind == 'dup7':
    return (r.randint(-3, 4, shape)).astype(dt)
  if kind == 'equal':
    return np.full(shape, -7, dt)
  if kind in ('asc', 'desc'):
    x = np.sort(sort_data(shape, dt, 'uniform', seed), axis=1)
    return x[:, ::-1, :].copy() if kind == 'desc' else x
  if kind == 'digit':
    # one random base pattern per line, digit `digit` replaced by random bytes
    if dt.kind == 'f':  # a finite, normal base whose digit can take any byte: exponent bits kept mid-range
      base = np.array([0x40490FDB if dt.itemsize == 4 else 0x400921FB54442D18], ut)
      if digit == key_bits(dt) // 8 - 1:  # the top digit holds the sign and exponent bits: avoid inf / NaN
        byte = r.randint(0, 0x7F, shape).astype(ut) + (r.randint(0, 2, shape).astype(ut) << ut(7))
      else:
        byte = r.randint(0, 256, shape).astype(ut)
    else:
      base = np.array([0x12345678 if dt.itemsize == 4 else 0x123456789ABCDEF0], ut)
      byte = r.randint(0, 256, shape).astype(ut)
    sh = ut(8 * digit)
    bits = (base & ~(ut(0xFF) << sh)) | (byte << sh)
    return bits.astype(ut).view(dt).reshape(shape)
  assert kind == 'extremes', kind
  if dt.kind == 'i':
    info = np.iinfo(dt)
    pool = np.array([info.min, -1, 0, info.max, info.min + 1, info.max - 1, 1], dt)
    return pool[r.randint(0, len(pool), shape)]
  x = (r.randint(-4, 5, shape) * 0.5).astype(dt)
  sp = np.array(FLOAT_SPECIALS[dt], dt)
  pick = r.random_sample(shape)
  x = np.where(pick < 0.25, sp[r.randint(0, len(sp), shape)], x)
  nans = np.array([_nan(dt, k & 1, 1 + k) for k in range(8)], dt)
  x = np.where(pick > 0.95, nans[r.randint(0, len(nans), shape)], x)
  return x.astype(dt)


def neg_zero_count(x, axis):
  """Number of -0.0 along ``axis``."""
  return np.sum((x == 0) & np.signbit(x), axis=axis)

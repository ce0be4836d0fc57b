"""Tile-wise NumPy restatement of the reference's scan (spartan/expr/scan.py:
24-64, 83-96), shared by tests/test_scan.py and tests/test_scan_gpu.py, and
the NumPy ``scan`` the CPU test double gets.

``scan_tiles`` walks the same tile grid a DistArray of that shape, tile hint
and worker count has: per-tile ``reduce_fn`` totals, ``scan_fn`` over the
totals, the base added to each tile's first slice, ``scan_fn`` over the tile
-- all in NumPy's own dtypes (an fp32 array is summed and scanned in fp32).
The one departure from the reference's text: a tile is converted to the
scan's result dtype before its base is added (the reference adds an int64 or
float base into a copy of the tile in the tile's dtype, which wraps for int32
and fails for bool)."""
import numpy as np

from spartan_amd import backend as B
from spartan_amd.array import distarray
from fake_backend import FakeBackend, _np, _put


def scan_tiles(a, axis, tile_hint, W, reduce_fn=np.sum, scan_fn=np.cumsum):
  a = np.asarray(a)
  nd = a.ndim
  ax = nd - 1 if axis is None else axis % nd
  exts = list(distarray.compute_extents(a.shape, tile_hint, W))
  cuts = sorted({(e.ul[ax], e.lr[ax]) for e in exts})
  tid = {u: i for i, (u, _) in enumerate(cuts)}
  probe = np.zeros((1,) * nd, a.dtype)
  tdt = np.asarray(reduce_fn(probe, axis=ax)).dtype
  odt = np.asarray(scan_fn(probe, axis=ax)).dtype
  tshape = tuple(len(cuts) if d == ax else a.shape[d] for d in range(nd))

  def where(e, t):
    return tuple(slice(t, t + 1) if d == ax else slice(e.ul[d], e.lr[d]) for d in range(nd))

  tot = np.zeros(tshape, tdt)
  for e in exts:
    tile = a[e.to_slice()]
    tot[where(e, tid[e.ul[ax]])] = np.asarray(reduce_fn(tile, axis=ax)).reshape(
        tuple(1 if d == ax else tile.shape[d] for d in range(nd)))
  if axis is None:
    flat = np.asarray(scan_fn(tot, axis=None)).reshape(-1)
    base = np.concatenate((np.zeros(1, flat.dtype), flat[:-1])).reshape(tshape)
  else:
    base = np.asarray(scan_fn(tot, axis=ax))
  out = np.empty(a.shape, odt)
  first = tuple(slice(0, 1) if d == ax else slice(None) for d in range(nd))
  for e in exts:
    tile = a[e.to_slice()].astype(odt)
    t = tid[e.ul[ax]]
    b = t if axis is None else t - 1
    if b >= 0:
      tile[first] += base[where(e, b)].astype(odt)
    out[e.to_slice()] = np.asarray(scan_fn(tile, axis=ax)).reshape(tile.shape)
  return out


def flat_cumsum(a, dtype=None):
  """The reference's meaning of axis=None: np.cumsum(a.ravel()) in a's shape."""
  a = np.asarray(a)
  return np.cumsum(a.reshape(-1), dtype=dtype).reshape(a.shape)


class ScanFakeBackend(FakeBackend):
  """FakeBackend + a NumPy ``scan`` with HipBackend.scan's signature and
  dtype rules (int64 / float64 accumulation, result rounded once)."""

  def scan(self, src, out, axis_geom, carry=None, totals=None, exclusive=False):
    o, n, i = (int(v) for v in axis_geom)
    odt, adt = B.scan_dtypes(B.np_dtype(src.dtype))
    assert src.is_contiguous() and src.numel() == o * n * i
    assert out is not None or totals is not None
    x = _np(src).reshape(o, n, i).astype(adt)
    inc = np.cumsum(x, axis=1)
    if totals is not None:
      assert B.np_dtype(totals.dtype) == adt and totals.numel() == o * i
      _put(totals, inc[:, -1, :])
    if out is not None:
      assert B.np_dtype(out.dtype) == odt and out.numel() == src.numel()
      r = np.concatenate((np.zeros((o, 1, i), adt), inc[:, :-1, :]), axis=1) if exclusive else inc
      if carry is not None:
        assert B.np_dtype(carry.dtype) == adt and carry.numel() == o * i
        r = r + _np(carry).reshape(o, 1, i)
      _put(out, r.astype(odt))
    self.calls.append('scan')


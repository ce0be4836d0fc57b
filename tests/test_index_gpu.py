"""GPU parity of take / compress: ``HipBackend.take`` (spx_take),
``compact_count`` / ``compact`` (spx_compact_count / spx_compact) against
NumPy, and ``spartan_amd.take`` / ``compress`` / ``a[mask]`` over tile
layouts.  Everything is exact and compared as bytes (``view(uint8)``): values
move as bit patterns.
"""
import numpy as np
import pytest

from index_ref import INDEX_KINDS, MASK_KINDS, bits, index_data, mask_data, values

pytestmark = pytest.mark.gpu

MAX_ELEMS = 1 << 21
DTYPES = [np.bool_, np.int32, np.int64, np.float32, np.float64]
INNERS = [1, 3, 4, 65]
OUTERS = [1, 5]
CANARY = {np.dtype(np.bool_): True, np.dtype(np.int32): -1234567, np.dtype(np.int64): -(1 << 40) - 5,
          np.dtype(np.float32): -777.25, np.dtype(np.float64): -777.25}


def _T():
  from spartan_amd import backend
  return backend.COMPACT_TILE


def _ns():
  T = _T()
  return [1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1031]


def _geoms(n, inner):
  """(kept, dropped) (outer, n, inner) cases of one (n, inner): products above
  2^21 elements are left out, so every case stays small."""
  all_ = [(o, n, inner) for o in OUTERS]
  kept = [g for g in all_ if g[0] * g[1] * g[2] <= MAX_ELEMS]
  return kept, len(all_) - len(kept)


def _path(inner, dt):
  """The kernel shape of a geometry (aligned pointers): one lane per element,
  16-byte vectors along the row, or elements along the row."""
  if inner == 1:
    return 'elem'
  return 'vec' if (inner * np.dtype(dt).itemsize) % 16 == 0 else 'scalar'


GEOM_PARAMS = [(ni, inner) for ni in range(11) for inner in INNERS]


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _empty(shape, dt):
  import torch
  from spartan_amd import backend
  return torch.empty(shape, dtype=backend.torch_dtype(dt), device='cuda')


def _same(got, want, msg=''):
  assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape, msg)
  np.testing.assert_array_equal(bits(got), bits(want), err_msg=str(msg))


# ----------------------------------------------------------------- compact
def _run_compact(be, x, mask, msg=''):
  """count + compact of one (outer, n, inner) input, twice; checked against
  NumPy by bytes.  ``mask`` is n uint8 bytes (any nonzero selects)."""
  import torch
  o, n, i = x.shape
  src, mk = _dev(x), _dev(mask)
  want = x[:, mask != 0, :]
  total, ws = be.compact_count(mk)
  assert total == np.count_nonzero(mask) == want.shape[1], msg
  out = _empty(want.shape, x.dtype)
  be.compact(src, mk, out, (o, n, i), ws)
  total2, ws2 = be.compact_count(mk.view(torch.bool))
  again = _empty(want.shape, x.dtype)
  be.compact(src, mk.view(torch.bool), again, (o, n, i), ws2)
  assert total2 == total
  assert torch.equal(out.view(torch.uint8), again.view(torch.uint8)), msg  # the same bits every run
  assert torch.equal(src.cpu().view(torch.uint8), torch.as_tensor(x).view(torch.uint8))  # input untouched
  assert torch.equal(mk.cpu(), torch.as_tensor(mask))
  _same(out.cpu().numpy(), want, msg)


@pytest.mark.parametrize('ni,inner', GEOM_PARAMS)
def test_backend_compact_geometries(gpu_workers, ni, inner):
  """Every geometry, every dtype; the mask kind rotates with the case so each
  kind meets each path."""
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  n = _ns()[ni]
  kept, _ = _geoms(n, inner)
  for gi, (o, n, i) in enumerate(kept):
    for k, dt in enumerate(DTYPES):
      for r in range(2):
        kind = MASK_KINDS[(ni + 2 * k + gi + 5 * r) % len(MASK_KINDS)]
        x = values((o, n, i), dt, 1000 * ni + 10 * inner + k)
        _run_compact(be, x, mask_data(n, kind, ni + k + r, _T()), (o, n, i, dt, kind))


@pytest.mark.parametrize('dt', DTYPES)
def test_backend_compact_every_mask_kind_on_every_path(gpu_workers, dt):
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  T = _T()
  # one tile; ragged tiles; vector rows wide enough for a wave per row and a column split; long scalar rows
  for (o, n, i) in ((3, 777, 1), (2, 3 * T + 77, 1), (2, T + 9, 4), (1, 2 * T + 5, 3), (2, 300, 512), (1, 70, 2049)):
    x = values((o, n, i), dt, 50 + i)
    for k, kind in enumerate(MASK_KINDS):
      _run_compact(be, x, mask_data(n, kind, 60 + k, T), (o, n, i, kind))


def test_compact_cases_cover_every_path(gpu_ctx):
  """The size cap drops a counted few of the geometries; every path (one
  lane per element, vector rows, scalar rows) keeps a single-tile and a ragged
  multi-tile size."""
  T = _T()
  ns = _ns()
  assert ns[-1] > 2 * T and ns[-1] % T != 0 and ns[7:10] == [T - 1, T, T + 1]
  seen, dropped = set(), 0
  for ni, inner in GEOM_PARAMS:
    kept, d = _geoms(ns[ni], inner)
    dropped += d
    for (o, n, i) in kept:
      for dt in DTYPES:
        seen.add((_path(i, dt), 'one' if n <= T else ('ragged' if n % T else 'even')))
  assert dropped == 1, dropped  # (5, 2T + 1031, 65) alone
  for path in ('elem', 'vec', 'scalar'):
    assert (path, 'one') in seen and (path, 'ragged') in seen, (path, seen)


# -------------------------------------------------------------------- take
def _run_take(be, x, idx, n_total, lo, pad, msg=''):
  """take of the block ``x`` = rows [lo, lo + n_local) of an axis of n_total
  into a canary-filled, possibly strided out; rows outside the window and
  the padding must keep the canary."""
  import torch
  o, nl, i = x.shape
  m = len(idx)
  ors, oos = i + pad, m * (i + pad) + 2 * pad
  src, ix = _dev(x), _dev(idx)
  can = np.full((o * oos + 1,), CANARY[x.dtype], x.dtype)
  want = can.copy()
  r = np.where(idx < 0, idx.astype(np.int64) + n_total, idx.astype(np.int64))
  for j in np.nonzero((r >= lo) & (r < lo + nl))[0]:
    for oo in range(o):
      want[oo * oos + j * ors:oo * oos + j * ors + i] = x[oo, r[j] - lo]
  out = _dev(can)
  be.take(src, ix, out, (o, nl, i), lo, n_total, (oos, ors) if pad else None)
  again = _dev(can)
  be.take(src, ix, again, (o, nl, i), lo, n_total, (oos, ors))
  assert torch.equal(out.view(torch.uint8), again.view(torch.uint8)), msg
  _same(src.cpu().numpy(), x, 'input untouched')
  _same(out.cpu().numpy(), want, msg)


@pytest.mark.parametrize('ni,inner', GEOM_PARAMS)
def test_backend_take_geometries(gpu_workers, ni, inner):
  """n_total, m and inner over the boundaries; int32 and int64 indices; the
  index kind rotates; whole blocks, windows, dense and strided outs."""
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  ns = _ns()
  n_total, m = ns[ni], ns[(3 * ni + 1) % len(ns)]
  for gi, o in enumerate(OUTERS):
    if o * max(n_total, m) * inner > MAX_ELEMS:
      continue
    for k, dt in enumerate(DTYPES):
      kind = INDEX_KINDS[(ni + k + gi) % len(INDEX_KINDS)]
      idt = (np.int64, np.int32)[(ni + k + gi) % 2]
      idx = index_data(n_total, m, kind, 100 * ni + k, idt)
      x = values((o, n_total, inner), dt, 1000 * ni + 10 * inner + k)
      _run_take(be, x, idx, n_total, 0, 0, (o, n_total, m, inner, dt, kind, 'whole'))
      lo = n_total // 3
      nl = max(0, min(n_total - lo, n_total // 2 + (k % 2)))
      _run_take(be, x[:, lo:lo + nl].copy(), idx, n_total, lo, (0, 4, 3)[k % 3],
                (o, n_total, m, inner, dt, kind, 'window', lo, nl))


@pytest.mark.parametrize('dt', DTYPES)
def test_backend_take_every_index_kind_on_every_path(gpu_workers, dt):
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  # lane per unit; a wave per row (scalar / vector units); a workgroup per row (scalar / vector)
  for (o, n, m, i) in ((2, 1000, 777, 1), (2, 300, 301, 3), (1, 300, 130, 4), (2, 90, 75, 65), (1, 50, 41, 1024),
                       (1, 9, 7, 2049), (2, 9, 6, 32768)):
    x = values((o, n, i), dt, 70 + i)
    for k, kind in enumerate(INDEX_KINDS):
      idx = index_data(n, m, kind, 80 + k, (np.int64, np.int32)[k % 2])
      _run_take(be, x, idx, n, 0, 0, (o, n, m, i, kind))
      _run_take(be, x[:, 2:n - 3].copy(), idx, n, 2, 16, (o, n, m, i, kind, 'window'))


@pytest.mark.parametrize('inner', [1, 3, 4, 65, 256, 2049])
def test_backend_take_out_of_range_raises_and_writes_nothing(gpu_workers, inner):
  gpu_workers(1)
  import torch
  from spartan_amd import backend
  be = backend.get()
  n, m = 300, 257
  for dt in (np.float32, np.int64):
    x = values((2, n, inner), dt, 5)
    for idt, bad_vals in ((np.int64, (n, -n - 1, 1 << 40)), (np.int32, (n, -n - 1, -(1 << 31)))):
      idx = index_data(n, m, 'random', 9, idt)
      bad = np.array([0, 63, 64, 200, m - 1])
      idx[bad] = np.resize(np.array(bad_vals, idt), len(bad))
      can = np.full((2, m, inner), CANARY[np.dtype(dt)], dt)
      out = _dev(can)
      with pytest.raises(IndexError):
        be.take(_dev(x), _dev(idx), out, (2, n, inner), 0, n)
      got = out.cpu().numpy()
      _same(got[:, bad], can[:, bad], 'bad rows keep the canary')
      good = np.setdiff1d(np.arange(m), bad)
      _same(got[:, good], x[:, idx[good].astype(np.int64) % n], 'the valid rows are gathered')
  # a block that owns nothing still range-checks
  e = torch.empty((0,), dtype=torch.float32, device='cuda')
  out = _dev(np.zeros(3, np.float32))
  be.take(e, _dev(np.array([0, -5, 4])), out, (1, 0, 1), 0, 5)
  with pytest.raises(IndexError):
    be.take(e, _dev(np.array([0, 5, 4])), out, (1, 0, 1), 0, 5)


# --------------------------------------------------------------- alignment
@pytest.mark.parametrize('dt', [np.float32, np.int64, np.bool_])
def test_unaligned_pointers(gpu_workers, dt):
  """Source, mask, index and out offset by one element, with a row length
  that is eligible for 16-byte vectors."""
  gpu_workers(1)
  import torch
  from spartan_amd import backend
  be = backend.get()
  T = _T()
  tdt = backend.torch_dtype(dt)

  def off1(a):
    buf = torch.empty((a.size + 1,), dtype=torch.as_tensor(a.reshape(-1)[:1]).dtype, device='cuda')
    v = buf[1:]
    v.copy_(_dev(a).reshape(-1))
    return v
  for (o, n, i) in ((2, T + 77, 16), (1, 300, 256), (2, 1000, 1)):
    x = values((o, n, i), dt, 3)
    mask = mask_data(n, 'half', 4)
    want = x[:, mask != 0, :]
    for us, um, uo in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
      src = off1(x) if us else _dev(x).reshape(-1)
      mk = off1(mask) if um else _dev(mask)
      out = (torch.empty((want.size + 1,), dtype=tdt, device='cuda')[1:] if uo
             else torch.empty((want.size,), dtype=tdt, device='cuda'))
      assert (src.data_ptr() % 16 != 0) == bool(us) and (mk.data_ptr() % 16 != 0) == bool(um)
      total, ws = be.compact_count(mk)
      assert total == want.shape[1]
      be.compact(src, mk, out, (o, n, i), ws)
      _same(out.cpu().numpy().reshape(want.shape), want, ('compact', o, n, i, us, um, uo))
    idx = index_data(n, 333, 'random', 5)
    wt = x[:, idx]
    for us, ui, uo in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
      src = off1(x) if us else _dev(x).reshape(-1)
      ix = off1(idx) if ui else _dev(idx)
      out = (torch.empty((wt.size + 1,), dtype=tdt, device='cuda')[1:] if uo
             else torch.empty((wt.size,), dtype=tdt, device='cuda'))
      be.take(src, ix, out, (o, n, i), 0, n)
      _same(out.cpu().numpy().reshape(wt.shape), wt, ('take', o, n, i, us, ui, uo))


# --------------------------------------------------------- argument checks
def test_backend_argument_checks(gpu_workers):
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  x = _dev(np.arange(12, dtype=np.float32))
  i64 = _dev(np.array([0, 1, 2]))
  out = _empty((3,), np.float32)
  for bad in (lambda: be.take(x, i64, out, (1, 13, 1), 0, 13),                      # src too short
              lambda: be.take(x.reshape(3, 4).t(), i64, out, (1, 12, 1), 0, 12),    # src not contiguous
              lambda: be.take(x, _dev(np.array([0.0, 1.0])), out, (1, 12, 1), 0, 12),  # float index
              lambda: be.take(x, i64.reshape(3, 1), out, (1, 12, 1), 0, 12),        # 2-d index
              lambda: be.take(x, i64, _empty((3,), np.float64), (1, 12, 1), 0, 12),  # out dtype
              lambda: be.take(x, i64, _empty((2,), np.float32), (1, 12, 1), 0, 12),  # out too short
              lambda: be.take(x, i64, out, (1, 12, 1), 0, 12, (3, 2)),              # strides past out
              lambda: be.take(x, i64, _empty((12,), np.float32), (1, 4, 3), 0, 4, (9, 2)),  # row stride < inner
              lambda: be.take(x, i64, out, (1, 12, 1), 5, 16),                      # window past the axis
              lambda: be.take(x, i64, out, (1, 12, 1), -1, 12),
              lambda: be.take(x, _dev(np.arange(12)), x, (1, 12, 1), 0, 12)):       # out is src
    with pytest.raises(ValueError):
      bad()
  mask = _dev(np.ones(12, np.uint8))
  total, ws = be.compact_count(mask)
  assert total == 12 and be.compact_count(mask[:0]) == (0, None)
  for bad in (lambda: be.compact_count(x),                                          # not bytes
              lambda: be.compact_count(_dev(np.ones((4, 6), np.uint8)).t()),        # not contiguous
              lambda: be.compact(x, mask, _empty((12,), np.float32), (1, 13, 1), ws),
              lambda: be.compact(x, mask[:11], _empty((11,), np.float32), (1, 12, 1), ws),
              lambda: be.compact(x, x, _empty((12,), np.float32), (1, 12, 1), ws),
              lambda: be.compact(x, mask, _empty((12,), np.float64), (1, 12, 1), ws),
              lambda: be.compact(x, mask, _empty((13,), np.float32), (1, 12, 1), ws),   # count > n
              lambda: be.compact(x, mask, _empty((7,), np.float32), (2, 6, 1), ws),     # not whole lines
              lambda: be.compact(x, mask, _empty((12,), np.float32), (1, 12, 1), None),
              lambda: be.compact(x, mask, _empty((12,), np.float32), (1, 12, 1), ws[:4]),
              lambda: be.compact(x, mask, x, (1, 12, 1), ws)):
    with pytest.raises(ValueError):
      bad()
  # a count smaller than the total (a caller's error) never writes past out
  few = _dev(np.full(8, -1.0, np.float32))
  be.compact(x, mask, few[:5], (1, 12, 1), ws)
  np.testing.assert_array_equal(few.cpu().numpy(), [0, 1, 2, 3, 4, -1, -1, -1])


# ------------------------------------------------------- expression level
def _expr_shapes():
  """The shapes and split hints of tests/test_sort_gpu.py::_expr_shapes."""
  from spartan_amd import backend
  L = backend.SORT_LDS_MAX
  return [((257, 4099), (64, 1000)), ((70001,), (9973,)), ((3, 50, 130), (2, 17, 48)), ((5 * L + 3,), (L + 5,))]


_REF = {}


def _ref(si, kind):
  """The input of one case and its masks / indices, made once."""
  key = (si, kind)
  if key not in _REF:
    shape = _expr_shapes()[si][0]
    a = values(shape, np.float64 if kind == 'f64' else np.int64, 31 + si)
    idx = [index_data(n, (n // 2 + 7, 5)[d % 2], 'random', 40 + d) for d, n in enumerate(shape)]
    cond = [mask_data(n, ('half', 'runs')[d % 2], 50 + d) != 0 for d, n in enumerate(shape)]
    mk = (mask_data(a.size, 'half', 60 + si, _T()) != 0).reshape(shape)
    _REF[key] = (a, idx, cond, mk)
  return _REF[key]


@pytest.mark.parametrize('kind', ['f64', 'int64'])
@pytest.mark.parametrize('si', [0, 1, 2, 3])
@pytest.mark.parametrize('W', [1, 3])
def test_expr_take_compress_mask(gpu_workers, W, si, kind):
  gpu_workers(W)
  from spartan_amd import expr
  shape, split = _expr_shapes()[si]
  a, idx, cond, mk = _ref(si, kind)
  if kind == 'f64':
    assert np.isnan(a).any() and (np.signbit(a) & (a == 0)).any()
  for hint in (None, split):
    x = expr.from_numpy(a, tile_hint=hint)
    for axis in range(len(shape)):
      e = expr.take(x, idx[axis], axis)
      assert e.shape == np.take(a, idx[axis], axis).shape and e.dtype == a.dtype
      _same(e.glom(), np.take(a, idx[axis], axis), (hint, axis, 'take'))
      c = expr.compress(cond[axis], x, axis)
      _same(c.glom(), np.compress(cond[axis], a, axis), (hint, axis, 'compress'))
    _same(x[expr.from_numpy(idx[0], tile_hint=(1001,))].glom(), a[idx[0]], (hint, 'a[i]'))
    _same(x[expr.from_numpy(mk, tile_hint=split)].glom(), a[mk], (hint, 'a[mask]'))
    flat = mk.reshape(-1)[:a.size - 13]
    _same(expr.compress(flat, x).glom(), np.compress(flat, a), (hint, 'flat'))


def test_expr_of_lazy_input_and_view(gpu_workers):
  gpu_workers(3)
  from spartan_amd import expr
  r = np.random.RandomState(3)
  a = r.randint(-1000, 1000, (130, 257)).astype(np.int32)
  k = r.randint(0, 50, 130).astype(np.int64)
  x = expr.from_numpy(a, tile_hint=(40, 100))
  kx = expr.from_numpy(k, tile_hint=(33,))
  i = expr.from_numpy(np.array([5, 0, -1, 5, 129]))
  _same((expr.take(x * 2, i) + 1).optimized().glom(), (a * 2)[[5, 0, -1, 5, 129]] + 1)
  _same((expr.compress(kx > 20, x * 2, axis=0) + 1).optimized().glom(), (a * 2)[k > 20] + 1)
  _same(x[expr.argsort(kx)].glom(), a[np.argsort(k, kind='stable')])
  _same(x[x > 500].glom(), a[a > 500])
  _same(x[kx == 7].optimized().glom(), a[k == 7])
  v = a[5:120, 3:250].T
  y = x[5:120, 3:250].T
  _same(expr.take(y, [0, -1, 17], 1).glom(), v[:, [0, -1, 17]])
  _same(expr.take(y, [0, -1, 17], 0).glom(), v[[0, -1, 17]])
  _same(expr.compress(v[0] > 0, y, 1).glom(), v[:, v[0] > 0])
  _same(y[y > 0].glom(), v[v > 0])
  _same(expr.take(expr.as_array(a) * 2, [4, 4, -1], 1).glom(), (a * 2)[:, [4, 4, -1]])
  _same(expr.compress(k > 20, expr.as_array(a) * 2, 0).glom(), (a * 2)[k > 20])
  with pytest.raises(IndexError):
    expr.take(x, [0, 130]).force()
  with pytest.raises(IndexError):
    expr.compress(np.ones(131, bool), x, 0).force()
  e = expr.compress(np.zeros(130, bool), x, 0)
  assert e.shape == (0, 257) and e.glom().dtype == np.int32

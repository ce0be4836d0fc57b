"""GPU parity of sort / argsort: ``HipBackend.sort`` (spx_sort: the LDS path
and the radix path, contiguous and strided lines) against NumPy, and
``spartan_amd.sort`` / ``argsort`` over tile layouts.

Everything is exact: ``out_idx`` equals ``np.argsort(kind='stable')`` bit for
bit; ``out_vals`` equals ``np.sort`` under ``assert_array_equal`` (NaNs equal,
``-0.0 == 0.0``) with the number of negative zeros per line preserved.
"""
import numpy as np
import pytest

from sort_ref import key_bits, neg_zero_count, sort_data

pytestmark = pytest.mark.gpu

MAX_ELEMS = 1 << 21
DTYPES = [np.bool_, np.int32, np.int64, np.float32, np.float64]
KINDS = ['uniform', 'dup7', 'equal', 'asc', 'desc', 'extremes']


def _LT():
  from spartan_amd import backend
  return backend.SORT_LDS_MAX, backend.SORT_TILE


def _ns():
  L, T = _LT()
  return [1, 2, 63, 64, 65, 255, 256, 257, L - 1, L, L + 1, 3 * L + 17, 2 * T + 1031]


INNERS = [1, 3, 65]
OUTERS = [1, 5]


def _geoms(n, inner):
  """The (outer, n, inner) cases of one (n, inner): products above 2^21
  elements are left out, so every case stays small."""
  return [(o, n, inner) for o in OUTERS if o * n * inner <= MAX_ELEMS]


GEOM_PARAMS = [(ni, inner) for ni, n in enumerate(_ns()) for inner in INNERS if _geoms(n, inner)]


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _empty(shape, dt):
  import torch
  from spartan_amd import backend
  return torch.empty(shape, dtype=backend.torch_dtype(dt), device='cuda')


def _check(x, vals, idx, both_v, both_i, ref=None):
  """The three call forms of one (outer, n, inner) input against NumPy."""
  want_i, want_v = ref if ref is not None else (np.argsort(x, axis=1, kind='stable'), np.sort(x, axis=1))
  assert idx.dtype == np.int64 and vals.dtype == x.dtype
  np.testing.assert_array_equal(idx, want_i)
  np.testing.assert_array_equal(both_i, want_i)
  for v in (vals, both_v):
    np.testing.assert_array_equal(v, want_v)
    if x.dtype.kind == 'f':
      np.testing.assert_array_equal(neg_zero_count(v, 1), neg_zero_count(x, 1))
  np.testing.assert_array_equal(np.take_along_axis(x, both_i, 1), both_v)
  if x.dtype.kind == 'f':
    # with indices the zeros keep input order, signs included; NaNs may be canonicalised
    t = np.take_along_axis(x, both_i, 1)
    ok = ~np.isnan(t)
    np.testing.assert_array_equal(np.signbit(t)[ok], np.signbit(both_v)[ok])


def _run(be, x):
  import torch
  o, n, i = x.shape
  src = _dev(x)
  vals, idx = _empty(x.shape, x.dtype), _empty(x.shape, np.int64)
  both_v, both_i = _empty(x.shape, x.dtype), _empty(x.shape, np.int64)
  be.sort(src, vals, None, (o, n, i))
  be.sort(src, None, idx, (o, n, i))
  be.sort(src, both_v, both_i, (o, n, i))
  again_v, again_i = _empty(x.shape, x.dtype), _empty(x.shape, np.int64)
  be.sort(src, again_v, again_i, (o, n, i))
  assert torch.equal(both_i, again_i)
  assert torch.equal(both_v.view(torch.uint8), again_v.view(torch.uint8))  # the same bits
  assert torch.equal(src.cpu().view(torch.uint8), torch.as_tensor(x).view(torch.uint8))  # input untouched
  return vals.cpu().numpy(), idx.cpu().numpy(), both_v.cpu().numpy(), both_i.cpu().numpy()


@pytest.mark.parametrize('ni,inner', GEOM_PARAMS)
def test_backend_sort_geometries(gpu_workers, ni, inner):
  """Every geometry, every dtype; the data kind rotates with the case so
  each kind meets each path, and 'extremes' (NaN, +-0, INT_MIN) meets all."""
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  for gi, (o, n, i) in enumerate(_geoms(_ns()[ni], inner)):
    for k, dt in enumerate(DTYPES):
      for kind in (KINDS[(ni + k + gi) % len(KINDS)], 'extremes'):
        x = sort_data((o, n, i), dt, kind, 1000 * ni + 10 * inner + k)
        _check(x, *_run(be, x))


@pytest.mark.parametrize('dt', DTYPES)
def test_backend_sort_every_kind_on_both_paths(gpu_workers, dt):
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  L, T = _LT()
  for (o, n, i) in ((3, 777, 1), (2, 300, 5), (2, T + L + 77, 1), (1, L + 9, 3)):
    for k, kind in enumerate(KINDS):
      x = sort_data((o, n, i), dt, kind, 50 + k)
      _check(x, *_run(be, x))


@pytest.mark.parametrize('dt', DTYPES)
def test_backend_sort_each_radix_digit_alone(gpu_workers, dt):
  """Keys that differ in one 8-bit digit only: a pass that did nothing, or
  was not stable, shows here (256 values over thousands of keys: ties)."""
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  L, T = _LT()
  for digit in range(key_bits(dt) // 8):
    for (o, n, i) in ((2, T + 3 * L + 5, 1), (1, L + 1, 3), (2, 300, 1)):
      x = sort_data((o, n, i), dt, 'digit', 7 + digit, digit=digit)
      if np.dtype(dt) != np.bool_:
        assert len(np.unique(x)) > 100 and np.isfinite(x.astype(np.float64)).all()
      _check(x, *_run(be, x))


def test_both_paths_run_for_both_layouts(gpu_ctx):
  """The geometries above hold an LDS and a radix case for inner == 1 and
  for inner > 1 (the library's own choice, read through backend.sort_plan)."""
  from spartan_amd import backend
  seen = set()
  for n in _ns():
    for inner in INNERS:
      for (o, n_, i) in _geoms(n, inner):
        for dt in DTYPES:
          path, passes = backend.sort_plan(o, n_, i, dt)
          assert (path == 'lds') == (n_ <= backend.SORT_LDS_MAX) and (passes > 0) == (path == 'radix')
          seen.add((path, 'row' if i == 1 else 'col'))
  assert seen == {('lds', 'row'), ('radix', 'row'), ('lds', 'col'), ('radix', 'col')}, seen
  L, T = _LT()
  assert _ns()[-1] > 2 * T and _ns()[-1] % T != 0  # three radix tiles, the last one ragged


@pytest.mark.parametrize('dt', [np.float32, np.int64])
def test_backend_sort_unaligned_pointers(gpu_workers, dt):
  """Input and outputs offset by one element."""
  gpu_workers(1)
  import torch
  from spartan_amd import backend
  be = backend.get()
  L, T = _LT()
  for (o, n, i) in ((3, 1028, 1), (1, T + 4, 1)):
    x = sort_data((o, n, i), dt, 'dup7', 5)
    buf = torch.empty((o * n * i + 1,), dtype=backend.torch_dtype(dt), device='cuda')
    src = buf[1:]
    src.copy_(_dev(x).reshape(-1))
    vals = _empty((o * n * i + 1,), dt)[1:]
    idx = _empty((o * n * i + 1,), np.int64)[1:]
    assert src.is_contiguous() and vals.is_contiguous() and idx.is_contiguous()
    assert src.data_ptr() % (4 * src.element_size()) != 0 and idx.data_ptr() % 16 != 0
    be.sort(src, vals, idx, (o, n, i))
    np.testing.assert_array_equal(vals.cpu().numpy().reshape(o, n, i), np.sort(x, axis=1))
    np.testing.assert_array_equal(idx.cpu().numpy().reshape(o, n, i), np.argsort(x, axis=1, kind='stable'))
    # aligned input, unaligned output
    vals2 = _empty((o * n * i + 1,), dt)[1:]
    be.sort(_dev(x), vals2, None, (o, n, i))
    assert torch.equal(vals2, vals)


def test_backend_sort_argument_checks(gpu_workers):
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  x = _dev(np.arange(12, dtype=np.float32))
  with pytest.raises(ValueError):
    be.sort(x, None, None, (1, 12, 1))
  with pytest.raises(ValueError):
    be.sort(x, x, None, (1, 12, 1))
  with pytest.raises(ValueError):
    be.sort(x, _empty((12,), np.float64), None, (1, 12, 1))
  with pytest.raises(ValueError):
    be.sort(x, None, _empty((12,), np.int32), (1, 12, 1))
  with pytest.raises(ValueError):
    be.sort(x, _empty((12,), np.float32), None, (1, 13, 1))
  with pytest.raises(ValueError):
    be.sort(x.reshape(3, 4).t(), _empty((12,), np.float32), None, (1, 12, 1))


# ------------------------------------------------------- expression level
def _expr_shapes():
  L, T = _LT()
  return [((257, 4099), (64, 1000)), ((70001,), (9973,)), ((3, 50, 130), (2, 17, 48)), ((5 * L + 3,), (L + 5,))]


def _expr_data(shape, kind, seed):
  if kind == 'int64':
    return sort_data((1, int(np.prod(shape)), 1), np.int64, 'uniform', seed).reshape(shape)
  if kind == 'f32_dup':
    return sort_data((1, int(np.prod(shape)), 1), np.float32, 'dup7', seed).reshape(shape)
  return sort_data((1, int(np.prod(shape)), 1), np.float64, 'extremes', seed).reshape(shape)


_REF = {}


def _ref(si, kind, axis):
  """(input, np.sort, stable np.argsort) of one case, computed once."""
  key = (si, kind, axis)
  if key not in _REF:
    a = _expr_data(_expr_shapes()[si][0], kind, 31 + si)
    _REF[key] = (a, np.sort(a, axis=axis), None if axis is None else np.argsort(a, axis=axis, kind='stable'))
  return _REF[key]


@pytest.mark.parametrize('kind', ['int64', 'f32_dup', 'f64_nan'])
@pytest.mark.parametrize('si', [0, 1, 2, 3])
@pytest.mark.parametrize('W', [1, 3])
def test_expr_sort(gpu_workers, W, si, kind):
  gpu_workers(W)
  from spartan_amd import expr
  shape, split = _expr_shapes()[si]
  for hint in (None, split):
    for axis in (None,) + tuple(range(len(shape))):
      a, want_v, want_i = _ref(si, kind, axis)
      x = expr.from_numpy(a, tile_hint=hint)
      e = expr.sort(x, axis=axis)
      got = e.glom()
      assert got.dtype == a.dtype == e.dtype and got.shape == want_v.shape == e.shape
      np.testing.assert_array_equal(got, want_v, err_msg='%s %s' % (hint, axis))
      if a.dtype.kind == 'f':
        np.testing.assert_array_equal(neg_zero_count(got, axis), neg_zero_count(a, axis))
      if axis is None:
        continue
      g = expr.argsort(x, axis=axis)
      idx = g.glom()
      assert idx.dtype == np.int64 == g.dtype and idx.shape == a.shape
      np.testing.assert_array_equal(idx, want_i, err_msg='%s %s' % (hint, axis))


def test_expr_sort_of_lazy_input_and_view(gpu_workers):
  gpu_workers(3)
  from spartan_amd import expr
  a = sort_data((1, 130 * 257, 1), np.int32, 'uniform', 3).reshape(130, 257) % 1000
  x = expr.from_numpy(a, tile_hint=(40, 100))
  np.testing.assert_array_equal((expr.sort(x * 2, axis=0) + 1).optimized().glom(), np.sort(a * 2, axis=0) + 1)
  v = a[5:120, 3:250].T
  np.testing.assert_array_equal(expr.sort(x[5:120, 3:250].T, axis=1).glom(), np.sort(v, axis=1))
  np.testing.assert_array_equal(expr.argsort(x[5:120, 3:250].T, axis=0).glom(), np.argsort(v, axis=0, kind='stable'))
  np.testing.assert_array_equal(expr.argsort(x.T).optimized().glom(), np.argsort(a.T, axis=1, kind='stable'))
  np.testing.assert_array_equal(expr.sort(x.T, axis=None).glom(), np.sort(a.T, axis=None))
  idx = expr.argpartition(x, 100, axis=1).glom()
  np.testing.assert_array_equal(np.take_along_axis(a, idx, 1)[:, 100], np.sort(a, axis=1)[:, 100])

"""GPU parity of the prefix scan: ``HipBackend.scan`` (spx_scan, both kernels
in both modes) against NumPy, and ``spartan_amd.scan`` over tile layouts
against the tile-wise restatement of the reference (scan_ref.scan_tiles).

Tolerances are the project's (tests/test_gpu_parity.py): integers and bool
bit-exact; floats through ``check_fp`` -- every element within 1e-5 (fp32) /
1e-12 (fp64) relative of the NumPy result in the array's dtype, or at least as
close to the exact (np.longdouble) value as that result is.  Signed fp64 data
is held to the a-priori bound of a summation of depth <= i instead:
|gpu - exact| <= i * 2^-53 * sum_{j<=i} |x_j| for element i of its line.
"""
import numpy as np
import pytest

from test_gpu_parity import check_fp

pytestmark = pytest.mark.gpu

MAX_ELEMS = 1 << 22
DTYPES = [np.int64, np.int32, np.bool_, np.float32, np.float64]
RTOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}


def _C():
  from spartan_amd import backend
  return backend.SCAN_CHUNK


def _ns():
  C = _C()
  return [1, 63, 64, 65, 257, C - 1, C, C + 1, 3 * C + 17]


INNERS = [1, 3, 64, 257]
OUTERS = [1, 5]


def _geoms(n, inner):
  """The (outer, n, inner) cases of one (n, inner): products above 2^22
  elements are left out, so every case stays small."""
  return [(o, n, inner) for o in OUTERS if o * n * inner <= MAX_ELEMS]


GEOM_PARAMS = [(ni, inner) for ni, n in enumerate(_ns()) for inner in INNERS if _geoms(n, inner)]


def _data(shape, dtype, seed, signed=False):
  r = np.random.RandomState(seed)
  dtype = np.dtype(dtype)
  if dtype == np.bool_:
    return r.randint(0, 2, shape) > 0
  if dtype == np.int32:
    return r.randint(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
  if dtype == np.int64:
    return r.randint(-2 ** 40, 2 ** 40, shape, dtype=np.int64)
  u = r.random_sample(shape)
  return (2.0 * u - 1.0 if signed else u).astype(dtype)


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _empty(shape, dt):
  import torch
  from spartan_amd import backend
  return torch.empty(shape, dtype=backend.torch_dtype(dt), device='cuda')


def _excl(inc, first):
  """Exclusive form of an inclusive (o, n, i) scan whose line starts at ``first``."""
  return np.concatenate((np.broadcast_to(first, inc[:, :1, :].shape).astype(inc.dtype), inc[:, :-1, :]), axis=1)


def _check_geometry(be, x, seed):
  """One (outer, n, inner) input through the four call forms."""
  from spartan_amd import backend
  o, n, i = x.shape
  dt = x.dtype
  odt, adt = backend.scan_dtypes(dt)
  r = np.random.RandomState(seed)
  if adt.kind == 'f':
    carry = (100.0 * r.random_sample((o, i))).astype(adt)
  else:
    carry = r.randint(-2 ** 45, 2 ** 45, (o, i), dtype=np.int64)
  src = _dev(x)
  dcarry = _dev(carry)
  out0, out1, out2 = _empty((o, n, i), odt), _empty((o, n, i), odt), _empty((o, n, i), odt)
  tot0, tot1 = _empty((o, i), adt), _empty((o, i), adt)
  be.scan(src, out0, (o, n, i), totals=tot0)                        # plain, with totals
  be.scan(src, out1, (o, n, i), carry=dcarry)                       # with a carry
  be.scan(src, out2, (o, n, i), carry=dcarry, exclusive=True)       # exclusive, with a carry
  be.scan(src, None, (o, n, i), carry=dcarry, totals=tot1)          # totals only (no carry in them)
  g0, g1, g2 = out0.cpu().numpy(), out1.cpu().numpy(), out2.cpu().numpy()
  t0, t1 = tot0.cpu().numpy(), tot1.cpu().numpy()
  assert g0.dtype == odt and t0.dtype == adt
  if adt.kind != 'f':
    np.testing.assert_array_equal(t0, t1)
    inc = np.cumsum(x, axis=1)
    assert inc.dtype == odt
    c = carry.reshape(o, 1, i)
    np.testing.assert_array_equal(g0, inc)
    np.testing.assert_array_equal(g1, inc + c)
    np.testing.assert_array_equal(g2, _excl(inc + c, c))
    np.testing.assert_array_equal(t0, inc[:, -1, :])
    return
  rtol = RTOL[np.dtype(dt)]
  ld = np.longdouble
  exact = np.cumsum(x.astype(ld), axis=1)
  cl = carry.astype(ld).reshape(o, 1, i)
  cpu = np.cumsum(x, axis=1)  # in the array's dtype
  xc = x.copy()
  xc[:, 0, :] += carry.astype(dt)  # the reference adds the base to the first slice, then scans
  cpu_c = np.cumsum(xc, axis=1)
  check_fp(g0, cpu, exact, rtol)
  check_fp(g1, cpu_c, exact + cl, rtol)
  check_fp(g2, _excl(cpu_c, carry.astype(dt).reshape(o, 1, i)), _excl(exact + cl, cl), rtol)
  # the totals-only pass sums in an order of its own: both forms by the fp64 rule
  for t in (t0, t1):
    check_fp(t, np.sum(x.astype(np.float64), axis=1), exact[:, -1, :], 1e-12)


@pytest.mark.parametrize('ni,inner', GEOM_PARAMS)
def test_backend_scan_geometries(gpu_workers, ni, inner):
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  for (o, n, i) in _geoms(_ns()[ni], inner):
    for k, dt in enumerate(DTYPES):
      _check_geometry(be, _data((o, n, i), dt, 1000 * ni + 10 * inner + k), 77 + k)


def test_both_kernels_run_in_both_modes(gpu_ctx):
  """The geometries above hold a line and a chunked case for inner == 1 and
  for inner > 1 (the library's own choice, read through backend.scan_plan)."""
  from spartan_amd import backend
  seen = set()
  for n in _ns():
    for inner in INNERS:
      for (o, n_, i) in _geoms(n, inner):
        mode, chunk = backend.scan_plan(o, n_, i, np.float32)
        assert chunk == (backend.SCAN_CHUNK if mode == 'chunked' else n_)
        seen.add((mode, 'row' if i == 1 else 'col'))
  assert seen == {('line', 'row'), ('chunked', 'row'), ('line', 'col'), ('chunked', 'col')}, seen


@pytest.mark.parametrize('dt', [np.float32, np.int64, np.bool_])
def test_backend_scan_unaligned_pointers(gpu_workers, dt):
  """Input and output offset by one element: the 4-element vector path is
  not taken (n is a multiple of 4, so only the pointers decide)."""
  gpu_workers(1)
  import torch
  from spartan_amd import backend
  be = backend.get()
  C = _C()
  for (o, n, i) in ((3, 1028, 1), (1, C + 4, 1), (1, 2 * C + 8, 1)):
    x = _data((o, n, i), dt, 5)
    odt, adt = backend.scan_dtypes(dt)
    buf = torch.empty((o * n * i + 1,), dtype=backend.torch_dtype(dt), device='cuda')
    src = buf[1:]
    src.copy_(_dev(x).reshape(-1))
    obuf = _empty((o * n * i + 1,), odt)
    out = obuf[1:]
    assert src.data_ptr() % (4 * src.element_size()) != 0 and src.is_contiguous()
    tot = _empty((o, i), adt)
    be.scan(src, out, (o, n, i), totals=tot)
    got = out.cpu().numpy().reshape(o, n, i)
    if np.dtype(dt).kind == 'f':
      check_fp(got, np.cumsum(x, axis=1), np.cumsum(x.astype(np.longdouble), axis=1), RTOL[np.dtype(dt)])
    else:
      np.testing.assert_array_equal(got, np.cumsum(x, axis=1))
      np.testing.assert_array_equal(tot.cpu().numpy(), np.sum(x, axis=1, dtype=np.int64))
    # aligned input, unaligned output
    out2 = _empty((o * n * i + 1,), odt)[1:]
    be.scan(_dev(x), out2, (o, n, i))
    assert torch.equal(out2, out)


def test_backend_scan_signed_and_deterministic(gpu_workers):
  """Signed data: fp32 by the close-or-better rule (fp64 accumulation gives
  the rounded exact prefix), fp64 by the a-priori bound; and the same call
  twice gives the same bits."""
  gpu_workers(1)
  import torch
  from spartan_amd import backend
  be = backend.get()
  C = _C()
  for (o, n, i) in ((5, 4099, 1), (1, 3 * C + 17, 1), (2, 1031, 257), (1, C + 1, 3)):
    for dt in (np.float32, np.float64):
      x = _data((o, n, i), dt, 9, signed=True)
      src = _dev(x)
      out, again = _empty((o, n, i), dt), _empty((o, n, i), dt)
      be.scan(src, out, (o, n, i))
      be.scan(src, again, (o, n, i))
      assert torch.equal(out, again)
      got = out.cpu().numpy()
      exact = np.cumsum(x.astype(np.longdouble), axis=1)
      if dt == np.float32:
        check_fp(got, np.cumsum(x, axis=1), exact, 1e-5)
      else:
        idx = np.arange(n, dtype=np.float64).reshape(1, n, 1)
        bound = idx * 2.0 ** -53 * np.cumsum(np.abs(x), axis=1)
        err = np.abs(got.astype(np.longdouble) - exact).astype(np.float64)
        assert (err <= bound).all(), float((err - bound).max())


# ------------------------------------------------------- expression level
def _expr_shapes():
  C = _C()
  return [((257, 4099), (64, 1000)), ((70001,), (9973,)), ((3, 50, 130), (2, 17, 48)), ((5 * C + 3,), (C + 5,))]


def _line_index(shape, axis):
  """0-based position of every element within its scan line."""
  if axis is None:
    return np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
  idx = np.arange(shape[axis], dtype=np.float64)
  return np.broadcast_to(idx.reshape([-1 if d == axis else 1 for d in range(len(shape))]), shape)


@pytest.mark.parametrize('kind', ['int64', 'bool', 'f32', 'f64', 'f32_signed', 'f64_signed'])
@pytest.mark.parametrize('si', [0, 1, 2, 3])
@pytest.mark.parametrize('W', [1, 3])
def test_expr_scan(gpu_workers, W, si, kind):
  gpu_workers(W)
  from spartan_amd import expr
  from scan_ref import flat_cumsum, scan_tiles
  shape, split = _expr_shapes()[si]
  signed = kind.endswith('_signed')
  dt = {'int64': np.int64, 'bool': np.bool_, 'f32': np.float32, 'f64': np.float64}[kind.split('_')[0]]
  a = _data(shape, dt, 31 + si, signed=signed)
  ld = np.longdouble
  for hint in (None, split):
    for axis in (None,) + tuple(range(len(shape))):
      e = expr.scan(expr.from_numpy(a, tile_hint=hint), axis=axis)
      got = e.glom()
      again = expr.scan(expr.from_numpy(a, tile_hint=hint), axis=axis).glom()
      np.testing.assert_array_equal(got, again)  # deterministic
      direct = flat_cumsum(a) if axis is None else np.cumsum(a, axis=axis)
      assert got.dtype == direct.dtype == e.dtype and got.shape == a.shape
      if np.dtype(dt).kind != 'f':
        np.testing.assert_array_equal(got, direct, err_msg='%s %s' % (hint, axis))
        continue
      exact = flat_cumsum(a, ld) if axis is None else np.cumsum(a.astype(ld), axis=axis)
      if kind == 'f64_signed':
        mag = flat_cumsum(np.abs(a)) if axis is None else np.cumsum(np.abs(a), axis=axis)
        bound = _line_index(shape, axis) * 2.0 ** -53 * mag
        err = np.abs(got.astype(ld) - exact).astype(np.float64)
        assert (err <= bound).all(), (hint, axis, float((err - bound).max()))
      else:
        check_fp(got, scan_tiles(a, axis, hint, W), exact, RTOL[np.dtype(dt)])


def test_expr_scan_of_lazy_input_and_view(gpu_workers):
  gpu_workers(3)
  from spartan_amd import expr
  a = _data((130, 257), np.int32, 3) % 1000
  x = expr.from_numpy(a, tile_hint=(40, 100))
  np.testing.assert_array_equal((expr.scan(x * 2, axis=0) + 1).optimized().glom(), np.cumsum(a * 2, axis=0) + 1)
  np.testing.assert_array_equal(expr.scan(x[5:120, 3:250].T, axis=1).glom(),
                                np.cumsum(a[5:120, 3:250].T, axis=1))
  np.testing.assert_array_equal(expr.scan(x.T).glom(), np.cumsum(a.T.reshape(-1)).reshape(257, 130))

"""GPU parity of stencil / maxpool: ``HipBackend.stencil`` (spx_stencil) and
``HipBackend.maxpool`` (spx_maxpool) against the NumPy contract of
tests/stencil_ref.py, and ``spartan_amd.expr.stencil`` over tile layouts.

Convolution of integer-valued inputs in [-4, 4] is exact in both dtypes (the
sums stay below 2^24: K <= 150 gives |out| <= 2400) and is compared with
``assert_array_equal`` for any summation order; normal data is held to
``|got - ref| <= tol * stencil_mag`` with the project's parity tolerances (1e-5
float32, 1e-12 float64), which for K <= 150 hold for any summation order
(150 * 2^-24 = 8.9e-6).  Pooling moves values unchanged and is compared with
``assert_array_equal`` (by value: max(-0.0, 0.0) is either).
"""
import numpy as np
import pytest

from stencil_ref import (convnet_ref, driver_benchmark, driver_test_convnet, driver_test_stencil, int_data, layouts,
                         maxpool_ref, normal_data, pool_data, stencil_mag, stencil_ref)

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
DTYPES = [np.bool_, np.int32, np.int64, np.float32, np.float64]
CANARY = {np.dtype(np.bool_): True, np.dtype(np.int32): -1234567, np.dtype(np.int64): -(1 << 40) - 5,
          np.dtype(np.float32): -777.25, np.dtype(np.float64): -777.25}
GUARD = 64  # canary elements after the output


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _guarded(shape, dt):
  """(buffer, view): a canary-filled device buffer of prod(shape) + GUARD
  elements and its leading part viewed as ``shape``."""
  import torch
  from spartan_amd import backend
  n = int(np.prod(shape))
  buf = torch.full((n + GUARD,), CANARY[np.dtype(dt)], dtype=backend.torch_dtype(dt), device='cuda')
  return buf, buf[:n].view(*shape)


def _guard_intact(buf, shape, dt):
  n = int(np.prod(shape))
  tail = buf[n:].cpu().numpy()
  np.testing.assert_array_equal(tail, np.full(GUARD, CANARY[np.dtype(dt)], dt))


def _run_stencil(be, a, f, msg=''):
  """One spx_stencil call into a guarded output, twice: the guard is intact,
  the inputs are unchanged and both runs give the same bits."""
  import torch
  n, c, w, h = a.shape
  shape = (n, f.shape[0], w, h)
  da, df = _dev(a), _dev(f)
  buf, out = _guarded(shape, a.dtype)
  be.stencil(da, df, out)
  buf2, out2 = _guarded(shape, a.dtype)
  be.stencil(da, df, out2)
  assert torch.equal(buf.view(torch.uint8), buf2.view(torch.uint8)), msg
  _guard_intact(buf, shape, a.dtype)
  np.testing.assert_array_equal(da.cpu().numpy(), a, err_msg='images changed %s' % (msg,))
  np.testing.assert_array_equal(df.cpu().numpy(), f, err_msg='filters changed %s' % (msg,))
  return out.cpu().numpy()


def _wh(size):
  """A (W, H) pair with W * H == size, W != H and H odd (H as large as a
  divisor allows; 1 for a prime or a power of two)."""
  if size == 1:
    return (1, 1)
  hs = [h for h in range(1, int(size ** 0.5) + 1, 2) if size % h == 0 and size // h != h]
  return (size // hs[-1], hs[-1])


def _split(k):
  """(C, fw, fh) with C * fw * fh == k: fw the smallest divisor > 1 of k (k for
  a prime), fh the smallest of the rest, C what is left -- 15: (1, 3, 5), 16:
  (4, 2, 2), 17: (1, 17, 1)."""
  sd = lambda n: next((d for d in range(2, n + 1) if n % d == 0), 1)
  fw = sd(k)
  fh = sd(k // fw)
  return (k // fw // fh, fw, fh)


def _k_cases(bk):
  """{K: (C, fw, fh)} for K in {1, bk - 1, bk, bk + 1}, 75 and 150."""
  cases = {1: (1, 1, 1), 75: (3, 5, 5), 150: (6, 5, 5)}
  for k in (bk - 1, bk, bk + 1):
    cases[k] = _split(k)
  return cases


@pytest.mark.parametrize('fi', [0, 1, 2, 3])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_backend_stencil_tile_boundaries_exact(gpu_workers, dt, fi):
  """F, W * H and K over the block tile's boundaries, N in {1, 3}: exact."""
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  bm, bn, bk = backend.stencil_plan(dt)
  F = [1, bm - 1, bm, bm + 1][fi]
  sizes = [1, bn - 1, bn, bn + 1, 2 * bn + 7]
  kc = _k_cases(bk)
  assert sorted(kc) == sorted({1, bk - 1, bk, bk + 1, 75, 150}) and all(c * a * b == k for k, (c, a, b) in kc.items())
  assert any(a != b for (_, a, b) in kc.values())
  big = 0
  for si, size in enumerate(sizes):
    W, H = _wh(size)
    assert W * H == size and H % 2 == 1 and (W != H or size == 1)
    for ki, (K, (C, fw, fh)) in enumerate(sorted(kc.items())):
      for N in (1, 3):
        a = int_data((N, C, W, H), dt, 100 * si + ki)
        f = int_data((F, C, fw, fh), dt, 7 + ki)
        got = _run_stencil(be, a, f, (F, W, H, C, fw, fh, N))
        want = stencil_ref(a, f)
        big = max(big, float(np.abs(want).max()))
        np.testing.assert_array_equal(got, want.astype(dt), err_msg=str((F, W, H, C, fw, fh, N)))
  assert big < 2 ** 24


@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_backend_stencil_clipping_exact(gpu_workers, dt):
  """Filters larger than the image (every tap past the first row / column is
  clipped), W = H = 1, rows and columns of one element, fw != fh."""
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  for (N, C, W, H, F, fw, fh) in ((2, 3, 1, 1, 5, 1, 1), (2, 3, 1, 1, 5, 4, 3), (1, 2, 3, 5, 4, 7, 9),
                                  (3, 2, 4, 7, 3, 4, 7), (1, 4, 1, 33, 2, 3, 5), (1, 4, 33, 1, 2, 5, 3),
                                  (2, 1, 9, 11, 70, 2, 12), (1, 5, 20, 13, 3, 21, 1), (1, 5, 20, 13, 3, 1, 14)):
    a = int_data((N, C, W, H), dt, W + H)
    f = int_data((F, C, fw, fh), dt, fw + fh)
    got = _run_stencil(be, a, f, (N, C, W, H, F, fw, fh))
    np.testing.assert_array_equal(got, stencil_ref(a, f).astype(dt), err_msg=str((N, C, W, H, F, fw, fh)))
    if fw > W and fh > H and W == 1 and H == 1:  # only the tap (0, 0) is inside
      np.testing.assert_array_equal(got[:, :, 0, 0], np.einsum('nc,fc->nf', a[:, :, 0, 0], f[:, :, 0, 0]))


@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_backend_stencil_normal_data(gpu_workers, dt):
  """Normal data, K <= 150: |got - ref| <= tol * sum of magnitudes."""
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  bm, bn, bk = backend.stencil_plan(dt)
  tol = TOL[np.dtype(dt)]
  for (N, C, W, H, F, fw, fh) in ((2, 3, 23, 19, bm + 3, 5, 5), (1, 6, 2 * bn // 17 + 1, 17, 7, 5, 5),
                                  (3, 1, 31, 9, bm, 1, 1), (1, 9, 12, 21, 33, 4, 4), (2, 16, 8, 65, 9, 3, 3)):
    assert C * fw * fh <= 150
    a = normal_data((N, C, W, H), dt, 3 * W + H)
    f = normal_data((F, C, fw, fh), dt, 5 * fw + fh)
    got = _run_stencil(be, a, f, (N, C, W, H, F, fw, fh)).astype(np.float64)
    ref, mag = stencil_ref(a, f), stencil_mag(a, f)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(mag, np.finfo(np.float64).tiny)).max())
    print('stencil normal %s %s: max |err| / mag = %.3g (tol %g)' % (np.dtype(dt).name, (N, C, W, H, F, fw, fh),
                                                                      worst, tol))
    assert (err <= tol * mag).all(), (N, C, W, H, F, fw, fh, worst)


def test_backend_stencil_argument_checks(gpu_workers):
  gpu_workers(1)
  import torch
  from spartan_amd import backend
  be = backend.get()
  a = _dev(np.ones((2, 3, 4, 5), np.float32))
  f = _dev(np.ones((6, 3, 2, 2), np.float32))
  out = torch.empty((2, 6, 4, 5), dtype=torch.float32, device='cuda')
  be.stencil(a, f, out)
  for bad in (lambda: be.stencil(a, f.double(), out), lambda: be.stencil(a.int(), f.int(), out.int()),
              lambda: be.stencil(a, f, out.double())):
    with pytest.raises(TypeError):
      bad()
  for bad in (lambda: be.stencil(a[0], f, out), lambda: be.stencil(a, f[:, :2], out),
              lambda: be.stencil(a, f, out[:1]), lambda: be.stencil(a.transpose(2, 3), f, out.transpose(2, 3)),
              lambda: be.stencil(a, f[:0], out[:, :0]), lambda: be.stencil(a, a, a),
              lambda: be.maxpool(a, out[:, :3], 0, 1), lambda: be.maxpool(a, out[:, :3], 1, 0),
              lambda: be.maxpool(a, out[:, :3], 2, 2), lambda: be.maxpool(a[0], out[0, :3], 1, 1),
              lambda: be.maxpool(a, a, 1, 1)):
    with pytest.raises(ValueError):
      bad()
  with pytest.raises(TypeError):
    be.maxpool(a, out[:, :3].double(), 1, 1)
  be.stencil(a[:0], f, out[:0])  # N == 0: nothing to do
  be.maxpool(a[:0], out[:0, :3], 1, 1)


# ----------------------------------------------------------------- maxpool
SIDES = [1, 2, 5, 8, 9, 65]


@pytest.mark.parametrize('dt', DTYPES)
def test_backend_maxpool(gpu_workers, dt):
  """The five dtypes, (pool, stride) over {1,2,3,4} x {1,2,3}, W and H in
  {1, 2, 5, 8, 9, 65}, N * C in {1, 5}; NaN and infinities for the floats;
  guard intact, input unchanged, the same bits on a second run."""
  gpu_workers(1)
  import torch
  from spartan_amd import backend
  be = backend.get()
  isf = np.dtype(dt).kind == 'f'
  for nc in ((1, 1), (5, 1), (1, 5)):
    for W in SIDES:
      for H in SIDES:
        a = pool_data(nc + (W, H), dt, 10 * W + H)
        if isf:
          r = np.random.RandomState(W * 100 + H)
          pick = r.random_sample(a.shape)
          a[pick < 0.08] = np.nan
          a[(pick >= 0.08) & (pick < 0.14)] = np.inf
          a[(pick >= 0.14) & (pick < 0.25)] = -np.inf
        da = _dev(a)
        for pool in (1, 2, 3, 4):
          for stride in (1, 2, 3):
            want = maxpool_ref(a, pool, stride)
            buf, out = _guarded(want.shape, dt)
            be.maxpool(da, out, pool, stride)
            got = out.cpu().numpy()
            np.testing.assert_array_equal(got, want, err_msg=str((nc, W, H, pool, stride)))
            _guard_intact(buf, want.shape, dt)
            if (W, H) in ((65, 65), (9, 65), (1, 1)):
              buf2, out2 = _guarded(want.shape, dt)
              be.maxpool(da, out2, pool, stride)
              assert torch.equal(buf.view(torch.uint8), buf2.view(torch.uint8))
        np.testing.assert_array_equal(da.cpu().numpy(), a)
  if isf:
    assert np.isnan(maxpool_ref(a, 2, 2)).any()


def test_backend_maxpool_large_window_and_stride(gpu_workers):
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  a = pool_data((2, 3, 9, 70), np.float32, 3)
  for pool, stride in ((9, 1), (100, 7), (2, 100), (70, 70), (1 << 40, 1 << 40)):
    want = maxpool_ref(a, min(pool, 100), min(stride, 100))
    buf, out = _guarded(want.shape, np.float32)
    be.maxpool(_dev(a), out, pool, stride)
    np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=str((pool, stride)))
    _guard_intact(buf, want.shape, np.float32)


# ------------------------------------------------------- expression level
@pytest.mark.parametrize('W', [1, 3])
def test_expr_reference_drivers(gpu_workers, W):
  gpu_workers(W)
  from spartan_amd import expr
  from spartan_amd.expr import stencil
  res, a, f = driver_test_stencil(expr, stencil, W)
  np.testing.assert_array_equal(res.glom(), stencil_ref(a, f))
  ints = lambda shape, seed: int_data(shape, np.float64, seed)
  for data in (None, ints):
    res, a, ws = driver_test_convnet(expr, stencil, W, data=data)
    np.testing.assert_array_equal(res.glom(), convnet_ref(a, ws))
    res, a, ws = driver_benchmark(expr, stencil, W, data=data)
    np.testing.assert_array_equal(res.glom(), convnet_ref(a, ws))


_REF = {}


def _layout_case():
  """The inputs of the layout test and their references, made once."""
  if not _REF:
    shape = (5, 4, 21, 19)
    a = int_data(shape, np.float64, 1)
    f = int_data((6, 4, 3, 4), np.float64, 2)
    b = pool_data(shape, np.int64, 3)
    _REF.update(shape=shape, a=a, f=f, b=b, conv=stencil_ref(a, f), pool=maxpool_ref(b, 3, 2))
  return _REF


@pytest.mark.parametrize('W', [1, 3])
def test_expr_layouts(gpu_workers, W):
  gpu_workers(W)
  from spartan_amd import expr
  from spartan_amd.expr import stencil
  r = _layout_case()
  for hint in layouts(r['shape']):
    x = expr.from_numpy(r['a'], tile_hint=hint)
    np.testing.assert_array_equal(stencil.stencil(x, r['f']).glom(), r['conv'], err_msg=str(hint))
    fx = expr.from_numpy(r['f'], tile_hint=(2, 4, 3, 2))
    np.testing.assert_array_equal(stencil.stencil(x * 1, fx).optimized().glom(), r['conv'], err_msg=str(hint))
    y = expr.from_numpy(r['b'], tile_hint=hint)
    got = stencil.maxpool(y, 3, 2).glom()
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, r['pool'], err_msg=str(hint))
  val = stencil.stencil(r['a'], r['f']).force()  # a host input: a replicated result
  assert val.replicated
  np.testing.assert_array_equal(val.glom(), r['conv'])
  assert stencil.stencil(np.empty((0, 4, 21, 19)), r['f']).glom().shape == (0, 6, 21, 19)


@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_expr_convnet_chain(gpu_workers, dt, W):
  """The convnet chain of the reference's test_convnet: integer data exact
  end to end (|values| stay below 2^24), and normal data layer by layer --
  every conv against the NumPy contract applied to ITS input as the GPU
  produced it, within tol * sum of magnitudes; every pool exact."""
  gpu_workers(W)
  from spartan_amd import expr
  from spartan_amd.expr import stencil
  res, a, ws = driver_test_convnet(expr, stencil, W, dtype=dt, data=lambda shape, seed: int_data(shape, dt, seed))
  assert res.dtype == dt
  want = convnet_ref(a, ws)
  assert np.abs(want).max() < 2 ** 24
  np.testing.assert_array_equal(res.glom(), want)
  tol = TOL[np.dtype(dt)]
  a = normal_data((4, 3, 16, 16), dt, 21)
  x = expr.from_numpy(a, tile_hint=(2, 3, 9, 9))
  prev = a
  for li, shape in enumerate(((4, 3, 5, 5), (4, 4, 5, 5), (4, 4, 5, 5))):
    w = normal_data(shape, dt, 30 + li)
    conv = stencil.stencil(x, expr.from_numpy(w), 2)
    got = conv.glom()
    assert got.dtype == dt
    ref, mag = stencil_ref(prev, w), stencil_mag(prev, w)
    assert (np.abs(got.astype(np.float64) - ref) <= tol * mag).all(), li
    x = stencil.maxpool(conv)
    prev = x.glom()
    np.testing.assert_array_equal(prev, maxpool_ref(got, 2, 2))
